#!/usr/bin/env python3
"""Generates goal_force_amd/csrc/gf_conv_a4_loop.inc: the K loop of the 4-wave direct 3x3x3 convolution of the Wan VAE's 192- and
384-channel levels (conv_a4_kernel, gf_conv_a4.hip) as ONE inline-asm statement with hand-allocated registers.

    python tools/gen_conv_a4.py            # rewrites the .inc (committed; the build does not run this)

The loop is the 4-wave GEMM's (tools/gen_gemm_a4.py: one wave per SIMD, accumulators in AGPRs, every LDS read, LDS-DMA piece,
counted wait and barrier at a fixed MFMA slot) with two changes:

  * the C tile is 256 rows x 192 columns (a wave = 128 x 96 = 8 x 6 MFMA tiles, 96 MFMAs per 64-wide K tile instead of 128):
    Cout = 192 and 384 are whole tiles (the 256-wide tile would run a quarter of its MFMAs on padding);
  * the A operand is the activation itself.  It lives in a ZERO-BORDERED buffer [2 + T, H + 2, W + 2, C] (two history frames in
    front: the causal padding; one pixel of zeros around every frame: the spatial padding), and GEMM row m is the padded position
    m = (t (H + 2) + y) (W + 2) + x.  Tap (dt, dy, dx) of row m is then the buffer row m + (dt (H + 2) + dy) (W + 2) + dx: a constant
    row shift per tap, no border test, no gather — the A tile of a K tile is 256 CONSECUTIVE buffer rows x 64 channels, fetched by
    the same `buffer_load ... lds` pieces as a plain GEMM's.  Along K = (dt, dy, dx, cin) the source advances by 128 bytes per K
    tile inside a pixel row's three taps (3 C contiguous channels), by `jr` at the end of such a run and by `jf` at the end of a
    frame's three runs: ten scalar instructions per K tile keep the two counters (no table, no memory access).
    Rows of the padded border are computed like any other and dropped by the epilogue (2.6 % of the rows at 120 x 208).

Slots of one iteration (96 MFMAs; tile t multiplies from registers, tile t+1 sits in the other LDS stage, tile t+2 is in flight):
  0..7    the 8 A fragments of k-sub-step 1 of tile t; lgkmcnt(0); barrier B1 at 11 -> the stage's A region is dead;
  12..40  one staging piece of A(t+2) every 4 MFMAs (8 pieces), the first six followed by one B fragment read of sub-step 1;
  46      barrier B2 -> the 6 pieces of B(t+2) (47, 51, .. 67; the one that would fall between the counted wait and its barrier moves);
  64      s_waitcnt vmcnt(n): everything older than this iteration's pieces has landed; barrier B3 -> the 8 + 6 fragments of
          k-sub-step 0 of tile t+1 from the other stage, one read every 2 slots.
"""
import os

import a4_loop
from a4_loop import S_WR, STAGE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "goal_force_amd", "csrc", "gf_conv_a4_loop.inc")

NI, NJ = 8, 6                                         # 16-row blocks of A, 16-column blocks of W per wave
NS = 2 * NI * NJ                                      # MFMA slots per K tile (two k-sub-steps of 32)
PA, PB = 8, 6                                         # staging pieces per wave and K tile: A 256 rows, W 192 rows (8 rows per piece)
S_T, S_R, S_STEPA, S_Q, S_J, S_RUN, S_JR, S_JF = 55, 58, 59, 68, 69, 70, 71, 72      # the A source's run / frame counters
CLOBBER_S = list(range(36, 60)) + list(range(60, 73))
V_FIRST = 128                                         # v[128:255] are the loop's fragment registers
# schedule parameters (the shipped values are the defaults; tools/conv_a4_variants.sh sweeps them into build/variants/)
DS = int(os.environ.get("CONV_A4_DS", "4"))           # MFMA slots between staging pieces
WAIT_SLOT = int(os.environ.get("CONV_A4_WAIT", "64")) # slot of the counted wait for tile t+1
RD_STEP = int(os.environ.get("CONV_A4_RDSTEP", "2"))  # slots between the sub-step-0 fragment reads behind it


def advance_a():
    """The A source's step to the next K tile: 128 bytes inside a run of 3 C / 64 tiles (a pixel row's three taps are contiguous),
    `jr` at the end of a run (next pixel row), `jf` at the end of a frame's third run (next frame).  R = tiles left in the run,
    Q = runs left in the frame."""
    return [f"s_sub_u32 s{S_R}, s{S_R}, 1", f"s_cmp_eq_u32 s{S_Q}, 1", f"s_cselect_b32 s{S_J}, s{S_JF}, s{S_JR}",
            f"s_cmp_eq_u32 s{S_R}, 0", f"s_cselect_b32 s{S_STEPA}, s{S_J}, 128", f"s_cselect_b32 s{S_R}, s{S_RUN}, s{S_R}",
            f"s_cselect_b32 s{S_T}, 1, 0", f"s_sub_u32 s{S_Q}, s{S_Q}, s{S_T}", f"s_cmp_eq_u32 s{S_Q}, 0",
            f"s_cselect_b32 s{S_Q}, 3, s{S_Q}"]


ADVANCE_V = [f"v_add_u32 %[voffA], s{S_STEPA}, %[voffA]", "v_add_u32 %[voffB], 0x80, %[voffB]"]


def gen():
    F = a4_loop.Loop(NI, NJ, PA, PB, advance_a() + ["s_nop 0"] + ADVANCE_V)
    at, half = F.at, NI * NJ
    L = F.prologue([f"s_mov_b32 s{S_RUN}, %[run]", f"s_mov_b32 s{S_R}, %[run]", f"s_mov_b32 s{S_Q}, 3",
                    f"s_mov_b32 s{S_JR}, %[jr]", f"s_mov_b32 s{S_JF}, %[jf]"], soff_interleaved=False)
    # B2: behind the last A piece and the last sub-step-1 read of B
    plan = F.plan_staging(1, DS, 1, WAIT_SLOT, lambda a: max(a[-1] + 3, a[NJ - 1] + 4) if DS != 4 else a[-1] + 6)
    a_slots, b2 = plan["a_slots"], plan["b2"]
    assert a_slots[NJ - 1] + 1 < b2 - 1 and a_slots[NJ - 1] + 1 < half - 2, "the sub-step-1 reads of B must land before the second half starts"
    if b2 - 1 >= half:                                     # the barrier sits in the second half: its MFMAs need the fragments earlier
        at(half - 2, "s_waitcnt lgkmcnt(0)")
    assert half <= WAIT_SLOT, "the counted wait sits behind the first half's MFMAs"
    F.plan_toggle_reads(half + 2)
    at(WAIT_SLOT, f"s_waitcnt vmcnt({plan['n_before']})")
    at(WAIT_SLOT + 1, "s_barrier")
    F.plan_next_reads(WAIT_SLOT + 2, RD_STEP)
    assert WAIT_SLOT + 2 + RD_STEP * (NI + NJ - 1) <= NS - 3
    adv = plan["b_slots"][-1] + 1                          # the staging position moves on only behind the iteration's last piece
    at(adv, f"s_xor_b32 s{S_WR}, s{S_WR}, {STAGE}", *advance_a()[:3])
    at(adv + 1, *advance_a()[3:7])
    at(adv + 2, *advance_a()[7:])
    at(adv + 4, *ADVANCE_V)
    assert adv + 4 < NS - 4
    L += F.body()
    a4_loop.check(L, NI, NJ, PA, PB)
    return L, dict(plan, adv=adv)


def emit(name, lines, plan):
    header = f"""// GENERATED by tools/gen_conv_a4.py — do not edit.  The K loop of conv_a4_kernel as one asm statement ({NS} MFMAs per K tile).
// slot plan: A pieces {plan['a_slots']}, W pieces {plan['b_slots']}, barriers {plan['b1']} / {plan['b2']} / {WAIT_SLOT + 1}, s_waitcnt vmcnt({plan['n_before']}) at {WAIT_SLOT}.
// operands: voffA/voffB (per-lane source byte offsets; A advances by 128 / jr / jf per K tile, W by 128), rdA0/rdA1/rdB0/rdB1 (LDS
// fragment read addresses of k-sub-steps 0/1, stage toggled by XOR 0x10000), aLo/aHi/nrA, bLo/bHi/nrB (tile row base + valid
// bytes), soA/stA, soB/stB (this wave's first row-group offset and the 32-row stride, bytes), ldsW (this wave's LDS write base in
// stage 0), nk (K tiles >= 1), run (K tiles per contiguous run = 3 C / 64), jr / jf (A's byte step at the end of a run / of a
// frame's third run).  Accumulators are left in a[(i*8+j)*4 + r] = C[16 i + lane%16][16 j + 4 (lane/16) + r], i < 8, j < 6."""
    return a4_loop.emit(name, lines, NS, header, ["voffA", "voffB", "rdA0", "rdA1", "rdB0", "rdB1"],
                        a4_loop.srd_operands("nk", "run", "jr", "jf"), CLOBBER_S, V_FIRST)


def main():
    lines, plan = gen()
    text = emit("GF_CONV_A4_LOOP_ASM", lines, plan)
    out = os.environ.get("CONV_A4_OUT", OUT)
    with open(out, "w") as f:
        f.write(text)
    print(f"wrote {out}: {plan}")


if __name__ == "__main__":
    main()
