"""The core of the 4-wave K-loop generators (tools/gen_gemm_a4.py, tools/gen_conv_a4.py; tools/gen_gemm_a4f8.py takes the register
plan and `emit`): one statement of the register plan, the instruction builders, the prologue, the first two thirds of an iteration's
slot plan, the drain, the replay of a finished loop (`check`) and the text of the .inc file.

The frame: 4 waves (wm, wn) in 2 x 2, a wave = NI x NJ tiles of v_mfma_f32_16x16x32_bf16 (operands swapped: D = W_frag x A_frag),
accumulators in a[(i * 8 + j) * 4 + r], fragments in v[128:255] (two k-sub-step sets per operand), LDS = 2 stages x (A tile | W tile) of
128-byte rows, staged by `buffer_load_dwordx4 ... offen lds` in 1-KiB pieces (PA / PB per wave and tile).  A K tile is NS = 2 NI NJ MFMA
slots; `Loop.at(slot, ...)` puts instructions behind the MFMA of a slot.  A generator describes its tile, its schedule parameters and
its source-advance step; what the numbers were measured to be is in the generators' docstrings.
"""

# ---- register plan -------------------------------------------------------------------------------------------------
A_K0, B_K0, A_K1, B_K1 = 128, 160, 192, 224          # fragment i of a set: v[base + 4 i : base + 4 i + 3]
SRD_A, SRD_B = 60, 64                                 # s[60:63], s[64:67]
SOFF_A, SOFF_B = 36, 44                               # s[36:43], s[44:51]: row-group offsets of this wave's pieces
S_M0SAVE, S_CNT, S_WR, S_NRA, S_NRB = 52, 53, 54, 56, 57
# s55, s58, s59 and s68.. hold the generator's own source-advance state
STAGE = 65536
B_TILE = 32768
FRAG_STEP = 2048                                      # LDS bytes between the fragments of consecutive 16-row blocks


def v4(base, i):
    return f"v[{base + 4 * i}:{base + 4 * i + 3}]"


def acc(i, j):
    b = (i * 8 + j) * 4                                # one numbering for every tile width: gf_agpr_read<(i * 8 + j) * 4 + r>
    return f"a[{b}:{b + 3}]"


def rd(dst_base, i, addr, extra=0):
    off = i * FRAG_STEP + extra
    return f"ds_read_b128 {v4(dst_base, i)}, {addr}" + (f" offset:{off}" if off else "")


class Loop:
    """ni, nj: 16-row blocks of A / 16-column blocks of W per wave; pa, pb: staging pieces per wave and K tile; piece_step: LDS bytes
    between a wave's consecutive pieces; advance: the instructions that move the staging position one K tile on (prologue form);
    j_outer: the MFMA's first source operand constant over ni MFMAs instead of the second."""

    def __init__(self, ni, nj, pa, pb, advance, piece_step=0x1000, j_outer=False):
        self.ni, self.nj, self.pa, self.pb = ni, nj, pa, pb
        self.half = ni * nj
        self.ns = 2 * self.half
        self.advance, self.piece_step, self.j_outer = advance, piece_step, j_outer
        self.ev = {}                      # MFMA slot -> instructions issued right after it

    # ---- instruction builders ------------------------------------------------------------------------------------------
    def mfma(self, half, g):
        i, j = (g % self.ni, g // self.ni) if self.j_outer else (g // self.nj, g % self.nj)
        a, b = (A_K0, B_K0) if half == 0 else (A_K1, B_K1)
        return f"v_mfma_f32_16x16x32_bf16 {acc(i, j)}, {v4(b, j)}, {v4(a, i)}, {acc(i, j)}"

    def dma(self, which, p, back_to_back=False):
        """One 1-KiB piece + the M0 step to the next piece's LDS address (an M0 write needs one wait state before the next LDS-DMA:
        in the loop the next piece is several MFMAs away, in the prologue an s_nop pads it)."""
        srd, soff, voff = (SRD_A, SOFF_A, "%[voffA]") if which == 0 else (SRD_B, SOFF_B, "%[voffB]")
        return [f"buffer_load_dwordx4 {voff}, s[{srd}:{srd + 3}], s{soff + p} offen lds", f"s_add_u32 m0, m0, {self.piece_step:#x}"] + \
            (["s_nop 0"] if back_to_back else [])

    def dma_tile(self, fill=None):
        """The pa + pb pieces of one tile (prologue): back to back, or — `fill`, pa + pb lists of instructions — each followed by its
        share of other work (tile 1 is staged between the zeroing of the accumulators: nothing waits for it yet, and a burst of
        LDS-DMA instructions is expensive)."""
        out = [f"s_mov_b32 m0, s{S_WR}", "s_nop 0"]
        for p in range(self.pa):
            out += self.dma(0, p, fill is None) + ([] if fill is None else fill[p])
        out += [f"s_add_u32 m0, s{S_WR}, {B_TILE}", "s_nop 0"]
        for p in range(self.pb):
            out += self.dma(1, p, fill is None) + ([] if fill is None else fill[self.pa + p])
        return out + self.advance

    # ---- prologue ------------------------------------------------------------------------------------------------------
    def prologue(self, setup, soff_interleaved, dense=False):
        """Descriptors, `setup` (the generator's source-advance state), the pieces' row-group offsets, tile 0 -> stage 0, tile 1 ->
        stage 1 (zeros past K) with the accumulators zeroed between its pieces (dense: behind them), the sub-step-0 fragments of tile 0."""
        pa, pb = self.pa, self.pb
        L = [f"s_mov_b32 s{S_M0SAVE}, m0"]
        L += [f"s_mov_b32 s{SRD_A}, %[aLo]", f"s_mov_b32 s{SRD_A + 1}, %[aHi]", f"s_mov_b32 s{SRD_A + 2}, %[nrA]",
              f"s_mov_b32 s{SRD_A + 3}, 0x00020000",
              f"s_mov_b32 s{SRD_B}, %[bLo]", f"s_mov_b32 s{SRD_B + 1}, %[bHi]", f"s_mov_b32 s{SRD_B + 2}, %[nrB]",
              f"s_mov_b32 s{SRD_B + 3}, 0x00020000",
              f"s_mov_b32 s{S_NRA}, %[nrA]", f"s_mov_b32 s{S_NRB}, %[nrB]", f"s_mov_b32 s{S_CNT}, %[nk]",
              f"s_mov_b32 s{S_WR}, %[ldsW]"] + setup
        L += [f"s_mov_b32 s{SOFF_A}, %[soA]", f"s_mov_b32 s{SOFF_B}, %[soB]"]
        step_a = [f"s_add_u32 s{SOFF_A + p}, s{SOFF_A + p - 1}, %[stA]" for p in range(1, pa)]
        step_b = [f"s_add_u32 s{SOFF_B + p}, s{SOFF_B + p - 1}, %[stB]" for p in range(1, pb)]
        L += [x for ab in zip(step_a, step_b) for x in ab] if soff_interleaved else step_a + step_b
        L += self.dma_tile()                                              # tile 0 -> stage 0
        L += [f"s_xor_b32 s{S_WR}, s{S_WR}, {STAGE}",
              f"s_cmp_gt_u32 s{S_CNT}, 1", f"s_cselect_b32 s{SRD_A + 2}, s{S_NRA}, 0", f"s_cselect_b32 s{SRD_B + 2}, s{S_NRB}, 0",
              "s_nop 1"]
        zero = [f"v_accvgpr_write_b32 a{(i * 8 + j) * 4 + r}, 0" for i in range(self.ni) for j in range(self.nj) for r in range(4)]
        if dense:                                                         # all pieces back to back, then the zeroing
            L += self.dma_tile() + [f"s_xor_b32 s{S_WR}, s{S_WR}, {STAGE}"] + zero
        else:
            n = pa + pb
            L += self.dma_tile([zero[q * len(zero) // n:(q + 1) * len(zero) // n] for q in range(n)])
            L += [f"s_xor_b32 s{S_WR}, s{S_WR}, {STAGE}"]
        L += [f"s_waitcnt vmcnt({pa + pb})", "s_barrier"]
        L += [rd(A_K0, i, "%[rdA0]") for i in range(self.ni)] + [rd(B_K0, j, "%[rdB0]") for j in range(self.nj)]
        return L + ["s_waitcnt lgkmcnt(0)"]

    # ---- the slot plan -------------------------------------------------------------------------------------------------
    def at(self, slot, *ins):
        assert 0 <= slot < self.ns, slot
        self.ev.setdefault(slot, []).extend(ins)

    def plan_staging(self, r1, ds, m0_late, wait_slot, b2_of):
        """Slots 0 .. the last piece: whether tile t+2 exists; the A fragments of sub-step 1 every r1 slots; barrier B1 (the stage's A
        region is dead); one piece of A(t+2) every ds slots, each of the first nj followed by one B fragment read of sub-step 1;
        barrier B2 at b2_of(a_slots); the pieces of W(t+2).  The M0 step of a piece sits m0_late slots behind it (the piece still has
        to read M0).  Returns the plan (a_slots, b_slots, b1, b2, n_before = pieces issued before the counted wait at wait_slot)."""
        at, pa, pb = self.at, self.pa, self.pb
        at(0, f"s_cmp_gt_u32 s{S_CNT}, 2", f"s_cselect_b32 s{SRD_A + 2}, s{S_NRA}, 0")       # tile t+2 exists iff remaining > 2
        at(1, f"s_cselect_b32 s{SRD_B + 2}, s{S_NRB}, 0")
        b1 = self.ni * r1 + 3                                 # B1: behind the last sub-step-1 read of A
        for i in range(self.ni):
            at(r1 * i, rd(A_K1, i, "%[rdA1]"))
        at(b1 - 2, f"s_mov_b32 m0, s{S_WR}")
        at(b1 - 1, "s_waitcnt lgkmcnt(0)")
        at(b1, "s_barrier")
        a_slots = [b1 + 1 + ds * p for p in range(pa)]
        b2 = b2_of(a_slots)                                   # B2: behind the last A piece and the last sub-step-1 read of B
        b_slots = [b2 + 1 + ds * p for p in range(pb)]
        b_slots = [x + 2 if x in (wait_slot, wait_slot + 1) else x for x in b_slots]    # not between the counted wait and its barrier
        for p in range(pa):
            at(a_slots[p], self.dma(0, p)[0])
            if p < self.nj:
                at(a_slots[p] + 1, rd(B_K1, p, "%[rdB1]"))
            if p < pa - 1:
                at(a_slots[p] + m0_late, self.dma(0, p)[1])
        assert b2 - 2 > a_slots[-1], "M0 moves to the W region only behind the last A piece"
        at(b2 - 2, f"s_add_u32 m0, s{S_WR}, {B_TILE}")
        at(b2 - 1, "s_waitcnt lgkmcnt(0)")
        at(b2, "s_barrier")
        for p in range(pb):
            at(b_slots[p], self.dma(1, p)[0])
            if p < pb - 1:
                at(b_slots[p] + m0_late, self.dma(1, p)[1])
        # pieces of this iteration that are issued before the counted wait: everything older than them (= all of tile t+1, including
        # the pieces the previous iteration issued behind ITS wait) has landed once vmcnt has dropped to their number
        n_before = sum(1 for x in a_slots + b_slots if x < wait_slot)
        assert a_slots[-1] < wait_slot, "the counted wait sits behind the A pieces"
        return dict(a_slots=a_slots, b_slots=b_slots, b1=b1, b2=b2, n_before=n_before)

    def plan_toggle_reads(self, slot):
        """The read addresses move to the other stage between the last sub-step-1 read and the first sub-step-0 read of the next tile."""
        self.at(slot, "v_xor_b32 %[rdA0], 0x10000, %[rdA0]", "v_xor_b32 %[rdA1], 0x10000, %[rdA1]")
        self.at(slot + 1, "v_xor_b32 %[rdB0], 0x10000, %[rdB0]", "v_xor_b32 %[rdB1], 0x10000, %[rdB1]")

    def plan_next_reads(self, first, step):
        """The sub-step-0 fragments of tile t+1 behind the counted wait and its barrier: A, then B, one read every `step` slots."""
        for i in range(self.ni):
            self.at(first + step * i, rd(A_K0, i, "%[rdA0]"))
        for j in range(self.nj):
            self.at(first + step * self.ni + step * j, rd(B_K0, j, "%[rdB0]"))

    def body(self, keep=lambda ins: True):
        """The loop with its closing count-down, then the drain: the last two iterations staged zero tiles; they must have landed
        (and every wave must be past its reads) before the epilogue reuses LDS.  MFMA results need 4 passes + margin before
        v_accvgpr_read."""
        ns = self.ns
        self.at(ns - 4, f"s_sub_u32 s{S_CNT}, s{S_CNT}, 1")
        self.at(ns - 3, f"s_cmp_eq_u32 s{S_CNT}, 0")
        self.at(ns - 2, "s_waitcnt lgkmcnt(0)")
        L = ["1:"]
        for s in range(ns):
            L.append(self.mfma(s // self.half, s % self.half))
            L += [ins for ins in self.ev.get(s, []) if keep(ins)]
        L += ["s_cbranch_scc0 1b"]
        return L + ["s_waitcnt vmcnt(0)", "s_nop 7", "s_nop 7", f"s_mov_b32 m0, s{S_M0SAVE}", "s_barrier"]


def check(lines, ni, nj, pa, pb, reread=()):
    """Replay the slot plan of a finished loop (ni x nj MFMA tiles per wave, pa + pb pieces per K tile): register sets are not
    overwritten while MFMAs still read them, SCC is not clobbered between a compare and its selects, and the loop-closing compare
    is the last SCC writer before the branch.  `reread`: first registers of sub-step-0 fragments that the plan loads from the
    CURRENT tile at the top of the iteration (before their first use, with an LDS wait in between) instead of from the next tile
    behind their last use."""
    loop = lines[lines.index("1:") + 1:lines.index("s_cbranch_scc0 1b")]
    slot = -1
    first_read_of, last_read_of = {}, {}  # fragment register -> first / last MFMA slot that reads it
    writes = []                           # (slot, first register) of ds_read destinations
    lgkm0 = []                            # slots of the full LDS waits
    for ins in loop:
        if ins.startswith("v_mfma"):
            slot += 1
            ops = ins.split(None, 1)[1].split(", ")
            for o in ops[1:3]:
                lo = int(o[2:o.index(":")])
                first_read_of.setdefault(lo, slot)
                last_read_of[lo] = slot
        elif ins.startswith("ds_read_b128"):
            writes.append((slot, int(ins.split()[1][2:].split(":")[0])))
        elif ins == "s_waitcnt lgkmcnt(0)":
            lgkm0.append(slot)
    assert slot == 2 * ni * nj - 1, ("MFMAs per K tile", slot + 1)
    for s, r in writes:
        sub1 = r >= A_K1                   # sub-step-1 sets are read by the second half's MFMAs, sub-step-0 sets by the first half's
        if sub1:
            assert s < ni * nj, ("a sub-step-1 fragment must be loaded during the first half", s, r)
        elif r in reread and s < first_read_of[r]:
            assert any(s < w < first_read_of[r] for w in lgkm0), ("a re-read fragment is used before its LDS wait", s, r)
        else:
            assert s >= last_read_of[r], ("a sub-step-0 fragment is overwritten while the first half still reads it", s, r)
    scc_writers = ("s_cmp", "s_sub_u32", "s_add_u32", "s_xor_b32", "s_lshl")
    tail = [i for i in loop if i.startswith(scc_writers) or i.startswith("s_cselect")]
    assert tail[-1].startswith("s_cmp_eq_u32 s%d, 0" % S_CNT), ("the loop-closing compare is not the last SCC writer before the branch", tail[-3:])
    pend = None
    for ins in loop:
        if ins.startswith("s_cmp"):
            pend = ins
        elif ins.startswith("s_cselect"):
            assert pend is not None, ("select without a live compare", ins)
        elif ins.startswith(scc_writers):
            pend = None
    assert sum(1 for i in loop if i.startswith("buffer_load_dwordx4")) == pa + pb
    assert sum(1 for i in loop if i.startswith("ds_read_b128")) == 2 * (ni + nj)


def emit(name, lines, n_mfma, header, outs, ins, clobber_s, v_first):
    """The .inc text: `header` (comment lines), then #define name(operands) asm volatile(lines : outs "+v" : ins : clobbers).  `ins` =
    lines of (operand, constraint); the macro's parameters are outs + ins in order."""
    got = sum(1 for l in lines if l.startswith("v_mfma"))
    assert got == n_mfma, got
    body = "\n".join(f'    "{l}\\n\\t"' for l in lines)
    vclob = ", ".join(f'"v{r}"' for r in range(v_first, 256))
    aclob = ", ".join(f'"a{r}"' for r in range(256))
    sclob = ", ".join(f'"s{r}"' for r in clobber_s)
    params = ", ".join(list(outs) + [o for line in ins for o, _ in line])
    out_ops = ", ".join(f'[{o}] "+v"({o})' for o in outs)
    in_ops = ", \\\n          ".join(", ".join(f'[{o}] "{c}"({o})' for o, c in line) for line in ins)
    return f"""{header}
#define {name}({params}) \\
    asm volatile( \\
{body.replace(chr(10), " " + chr(92) + chr(10))} \\
        : {out_ops} \\
        : {in_ops} \\
        : "memory", "scc", "vcc", {sclob}, \\
          {vclob}, \\
          {aclob})
"""


def srd_operands(*tail):
    """The operand lines every loop ends on: tile bases + valid bytes, row-group offsets, LDS write base, then the generator's own."""
    return [[(o, "s") for o in ("aLo", "aHi", "nrA", "bLo", "bHi", "nrB", "soA")],
            [(o, "s") for o in ("stA", "soB", "stB", "ldsW") + tail]]
