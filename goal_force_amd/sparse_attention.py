"""Block-sparse self-attention patterns for the DiT / ControlNet blocks (dit.enable_sparse_attention).

The mechanism is ops.flash_attn_sparse: kernel 3 over a list of 64-key tiles per 256-row query block (ops.BlockMap).  A pattern
is any callable `grid -> ops.BlockMap`, grid = the (f, h, w) token grid of the latent video; the blocks ask it for the map of the
grid they run on.  Two families ship.  FrameWindow is static: it needs no token reordering, because the DiT's tokens are already
in (f, h, w) order and a window of frames is then a band of tiles.  MassCover is data-dependent: the blocks hand it the finished
q and k of every self-attention (`from_qk`), and it builds, on the device, per head the smallest set of tiles whose ESTIMATED
softmax mass reaches a requested share (ops.block_map_from_qk; the recipe is stated in include/goalforce.h).

The reference has no counterpart (its flash_attention is dense on every backend), so nothing here is pinned against it, and
what a sparse pattern does to the videos of a trained checkpoint is NOT measured in this repository: the switch
is off by default and the tests pin the mechanism — which keys a row sees, and that it sees them with the dense kernel's bits.
"""
from __future__ import annotations

import torch

from . import ops
from ._lib import GoalForceError

__all__ = ["FrameWindow", "MassCover", "frame_window_mask"]


def _check_grid(grid):
    try:
        f, h, w = (int(x) for x in grid)
    except (TypeError, ValueError):
        raise GoalForceError(f"sparse attention: expected a token grid (f, h, w), got {grid!r}") from None
    if min(f, h, w) < 1:
        raise GoalForceError(f"sparse attention: expected a token grid (f, h, w) of positive sizes, got {grid!r}")
    return f, h, w


def frame_window_mask(grid, window: int, sink_frames: int = 1) -> torch.Tensor:
    """The FrameWindow selection as a CPU bool array [n_qblocks, n_tiles] (the definition is FrameWindow's docstring).  Tokens are
    in frame order, so a block and a tile each cover an INTERVAL of frames and "some frame of the block and some frame of the tile
    are within `window`" is a test on the intervals' ends."""
    f, h, w = _check_grid(grid)
    S, hw = f * h * w, h * w
    qb, kb = ops.SPARSE_QB, ops.SPARSE_KB

    def frames(step):
        first = torch.arange(0, S, step)
        last = torch.clamp(first + step, max=S) - 1
        return first // hw, last // hw

    q_lo, q_hi = frames(qb)
    k_lo, k_hi = frames(kb)
    near = (k_lo[None, :] - q_hi[:, None] <= window) & (q_lo[:, None] - k_hi[None, :] <= window)
    return near | (k_lo[None, :] < sink_frames)


class FrameWindow:
    """Spatio-temporally local attention as a block-level cover: every query sees the keys of the frames within `window` of its
    own, plus the first `sink_frames` frames, rounded OUT to whole blocks.  Exactly, for a token grid (f, h, w), S = f h w tokens
    in (f, h, w) order:
      * a token's frame is token // (h * w);
      * query block b covers tokens [256 b, min(256 b + 256, S));
      * tile t covers tokens [64 t, min(64 t + 64, S));
      * (b, t) is selected iff some frame fq of the block and some frame fk of the tile satisfy |fq - fk| <= window or
        fk < sink_frames.
    So a query also sees the rest of every tile its window touches, and everything its block neighbours see (never less than the
    token-level window).  One map for all heads.  `pattern(grid)` returns the host-validated ops.BlockMap, `pattern(grid, device)`
    the copy on that device; both are memoised per (grid, device)."""

    def __init__(self, window: int, sink_frames: int = 1):
        if int(window) != window or window < 0 or int(sink_frames) != sink_frames or sink_frames < 0:
            raise GoalForceError(f"FrameWindow: expected non-negative integers, got window={window!r}, sink_frames={sink_frames!r}")
        self.window, self.sink_frames = int(window), int(sink_frames)
        self._maps = {}

    def __repr__(self):
        return f"FrameWindow({self.window}, {self.sink_frames})"

    def mask(self, grid) -> torch.Tensor:
        return frame_window_mask(grid, self.window, self.sink_frames)

    def __call__(self, grid, device=None) -> ops.BlockMap:
        grid = _check_grid(grid)
        key = (grid, None if device is None else str(torch.device(device)))
        if key not in self._maps:
            if (grid, None) not in self._maps:
                self._maps[(grid, None)] = ops.BlockMap(self.mask(grid))
            self._maps[key] = self._maps[(grid, None)].to(device) if device is not None else self._maps[(grid, None)]
        return self._maps[key]


class MassCover:
    """Data-dependent sparse attention: before every self-attention, q is pooled per 256-row query block and k per 64-key tile, every
    (block, tile) pair is scored with the pooled vectors, and per head and query block the smallest top set of tiles whose estimated
    share of the row's softmax mass reaches `mass` is kept (at least 2 tiles; ties taken together; a row with a non-finite score
    keeps everything) — ops.block_map_from_qk, on the attention's stream, with no host round trip.  `always`: a static pattern
    (a FrameWindow, or any callable grid -> ops.BlockMap of one map) whose tiles are kept whatever their score, or None.
    `mass` = 1 keeps every tile: the dense kernel's bits.  Flat attention degrades towards the dense map (density ~ mass), peaky
    attention keeps few tiles.  The mass is an ESTIMATE from pooled vectors (a Jensen lower bound of each tile's mass seen from the
    block's mean query), not a guarantee for the block's actual rows; the true retained mass of a run is 2^(lse_sparse - lse_dense)
    (tools/adaptive_map_bench.py measures it).  `keep_last`: the last built map stays as `.last_map` (tests, the bench).
    The blocks call `from_qk(q, k, num_heads, grid, scale)`; there is no map without q and k, so `pattern(grid)` is refused.
    `q_coherence` / `k_coherence` (numbers in (0, 1], or None): the coherence gate.  A pooled mean describes its rows only when they
    resemble each other; rho = |mean|^2 / mean(|row|^2) of a block measures that (1: equal rows).  A query block with rho below
    q_coherence keeps every tile; a key tile with rho below k_coherence is kept by every row of its head (as an `always` tile).
    GUARANTEED: if every ungated query block has equal rows and every unforced key tile has equal keys, every row's true retained
    mass is >= mass (the estimate is exact on the unforced tiles and a Jensen lower bound on the forced ones; gated rows retain 1) —
    thresholds near 1 predict only for constant blocks.  Below that, and with no gate, the mass stays an ESTIMATE to be measured;
    incoherent data (random q, k: rho ~ 1/n) degrades the gated map to dense."""

    def __init__(self, mass: float, always=None, keep_last: bool = False, q_coherence=None, k_coherence=None):
        try:
            ok = 0.0 < float(mass) <= 1.0
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise GoalForceError(f"MassCover: expected 0 < mass <= 1, got mass={mass!r}")
        if always is not None and not callable(always):
            raise GoalForceError(f"MassCover: expected `always` to be a static pattern grid -> ops.BlockMap (or None), got {type(always).__name__}")
        if hasattr(always, "from_qk"):
            raise GoalForceError(f"MassCover: expected `always` to be a static pattern, got the data-dependent {always!r}")
        self.mass, self.always, self.keep_last = float(mass), always, bool(keep_last)
        self.q_coherence = ops._block_map_min("MassCover", "q_coherence", q_coherence)
        self.k_coherence = ops._block_map_min("MassCover", "k_coherence", k_coherence)
        self.last_map = None

    def __repr__(self):
        if self.q_coherence is None and self.k_coherence is None:
            return f"MassCover({self.mass}, always={self.always!r})"
        return f"MassCover({self.mass}, always={self.always!r}, q_coherence={self.q_coherence}, k_coherence={self.k_coherence})"

    def __call__(self, grid, device=None):
        raise GoalForceError(f"{self!r} has no map without q and k: the blocks call from_qk(q, k, num_heads, grid, scale)")

    def from_qk(self, q, k, num_heads, grid, scale=None) -> ops.BlockMap:
        """The map of one self-attention on its finished q and k (after norm + RoPE, pre-scaled or not: `scale` is the softmax scale
        the attention is then called with)."""
        always = None
        if self.always is not None:
            always = self.always(_check_grid(grid))
            if not isinstance(always, ops.BlockMap):
                raise GoalForceError(f"MassCover: expected `always` to return an ops.BlockMap, got {type(always).__name__}")
        block_map = ops.block_map_from_qk(q, k, num_heads, self.mass, always=always, scale=scale, q_min=self.q_coherence,
                                          k_min=self.k_coherence)
        if self.keep_last:
            self.last_map = block_map
        return block_map
