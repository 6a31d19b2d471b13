"""Test helper: the cases of the fused branch merge (``csrc/tile_merge_tta.hip``), shared by the CPU test of its
restatement against the two-launch chain (tests/test_sliced_tta_cpu.py) and the GPU test of the kernel against the
restatement (tests/test_gpu_sliced_tta.py).

Layout as tests/test_gpu_sliced.py's merge case: F = 2, S = 3, two model calls of 3 + 2 tiles, six descriptor rows, one
of them an empty slot, one a whole-frame slot with gain 128 / 300 and a pad, rows with mixed interior flags. A call is
K = 3 branch outputs. Branch set "a" is the plan of a 128 x 128 canvas (A_tot 2893: odd, as at the real shapes), set
"b" a small odd one with an exact division, an upscale and both flips."""
from __future__ import annotations

import numpy as np

from tile_merge_tta_ref import tile_merge_tta_ref

F32 = np.float32
ALL = (True, True, True, True)
NONE = (False, False, False, False)
CANVAS = (128, 128)
# name -> [(A_k, (src_lo, n_k, dst_k, scale, flip))], A_tot
BRANCH_SETS = {
    "a": ([(1360, (0, 1344, 0, 1.0, None)), (1360, (0, 1360, 1344, 0.83, 3)), (765, (576, 189, 2704, 0.67, None))],
          2893),
    "b": ([(85, (0, 84, 0, 1.0, 2)), (52, (0, 52, 84, 0.5, 3)), (40, (29, 11, 136, 1.5, None))], 147),
}
FRAMES, SLOTS = 2, 3
MARGINS = (0.0, 2.0)
SIDES = ("left", "top", "right", "bottom")
EDGE_ROW = (0, 0, 0, 1.0, 0, 0, 0, 0, 128, 128, ALL)  # gain 1, pad 0, offset 0: merged holds bx, by, bw, bh themselves
N_EDGE = len(MARGINS) * len(SIDES) * 3  # anchor ((margin * 4 + side) * 3 + t), t = on the boundary, below it, above it


def calls_rows():
    g = 128 / 300
    return [
        [(0, 0, 0, 1.0, 0, 0, 0, 0, 128, 128, ALL),
         (1, 0, 2, g, 0, 21, 0, 0, 300, 200, NONE),                       # whole-frame slot of a (200, 300) frame
         (2, 1, 1, 1.0, 0, 0, 96, 72, 128, 128, (True, False, False, True))],
        [(0, 1, 0, 1.0, 0, 0, 172, 0, 128, 128, (False, True, True, False)),
         (-1, 0, 1, 1.0, 0, 0, 0, 0, 0, 0, NONE),
         (1, 1, 2, 128 / 150, 0, 25, 22, 3, 150, 90, ALL)],
    ]


def _step(v, k):
    """v moved by k fp32 steps (v > 0, no zero crossing)."""
    return (np.asarray(v, dtype=F32).view(np.int32) + np.int32(k)).view(F32)


def _edges(v, w, side, branch):
    """The restated edge that ``side``'s comparison reads, for boxes whose coordinate on that side's axis is ``v`` and
    whose extent along it is ``w`` (view pixels; the other axis: centre 64, extent 10 in tile pixels), through
    ``tile_merge_tta_ref`` itself on a gain-1 / pad-0 / offset-0 row."""
    scale = F32(branch[3])
    n = v.size
    mid, ten = F32(64) * scale, F32(10) * scale  # a centre that a flip leaves in the middle
    y = np.zeros((1, 5, n), dtype=F32)
    if side in ("left", "right"):
        y[0, 0], y[0, 1], y[0, 2], y[0, 3] = v, mid, w, ten
    else:
        y[0, 0], y[0, 1], y[0, 2], y[0, 3] = mid, v, ten, w
    m = tile_merge_tta_ref(y, [EDGE_ROW], np.full((1, 5, n), np.nan, dtype=F32), n, (0, n, 0, branch[3], branch[4]),
                           CANVAS, None)[0]
    c, e = (m[0], m[2]) if side in ("left", "right") else (m[1], m[3])
    return c - F32(0.5) * e if side in ("left", "top") else c + F32(0.5) * e


def boundary_boxes(branch):
    """[4, N_EDGE] (x, y, w, h) in the branch's view pixels for a 128 x 128 tile with gain 1 and pad 0: for each margin
    and each of the four comparisons a box whose de-scaled, de-flipped edge is exactly the comparison's boundary
    (margin, or 128 - margin), and its two neighbours: the nearest fp32 input to either side whose edge is below /
    above the boundary. Found by searching neighbouring floats on the restatement."""
    scale, flip = F32(branch[3]), branch[4]
    out = np.empty((4, N_EDGE), dtype=F32)
    R = 96
    for mi, m in enumerate(MARGINS):
        for si, side in enumerate(SIDES):
            target = F32(m) if side in ("left", "top") else F32(128 - m)
            tile_c = F32(5 + m) if side in ("left", "top") else F32(123 - m)   # the box's centre in tile pixels
            flipped = (flip == 3 and side in ("left", "right")) or (flip == 2 and side in ("top", "bottom"))
            v0 = ((F32(128) - tile_c) if flipped else tile_c) * scale
            w0 = F32(10) * scale
            k = np.arange(-R, R + 1)
            vs, ws = np.meshgrid(_step(v0, k), _step(w0, k), indexing="ij")
            e = _edges(vs.ravel(), ws.ravel(), side, branch).reshape(vs.shape)
            hit = np.argwhere(e == target)
            assert len(hit), f"no box with its {side} edge exactly on {target} near {v0} (scale {scale}, flip {flip})"
            i, j = hit[len(hit) // 2]
            v, w = vs[i, j], ws[i, j]
            line = _edges(_step(v, k), np.full(k.size, w, dtype=F32), side, branch)
            assert line[R] == target
            below = [d for d in sorted(k, key=abs) if line[R + d] < target][0]
            above = [d for d in sorted(k, key=abs) if line[R + d] > target][0]
            mid, ten = F32(64) * scale, F32(10) * scale
            for t, d in enumerate((0, below, above)):
                vv = _step(v, d)
                box = (vv, mid, w, ten) if side in ("left", "right") else (mid, vv, ten, w)
                out[:, (mi * len(SIDES) + si) * 3 + t] = box
    return out


def merge_tta_case(name, nc, seed=None):
    """``(ys, rows, branches, A_tot)``: ``ys[call][k]`` [n, 4+nc, A_k] float32 in the view's pixels, ``rows[call]`` the
    descriptor rows, ``branches[k]`` = (src_lo, n_k, dst_k, scale, flip). In set "a" the gain-1 / pad-0 source rows
    carry :func:`boundary_boxes` in the first ``N_EDGE`` kept anchors of every branch."""
    bs, A_tot = BRANCH_SETS[name]
    rng = np.random.default_rng(1000 * nc + len(name) + ord(name[0]) if seed is None else seed)
    no = 4 + nc
    ys = []
    for n in (3, 2):
        call = []
        for A_k, b in bs:
            s = F32(b[3])
            y = np.empty((n, no, A_k), dtype=F32)
            y[:, 0:2] = rng.uniform(-4, 132, (n, 2, A_k)).astype(F32) * s
            y[:, 2:4] = rng.uniform(0.5, 40, (n, 2, A_k)).astype(F32) * s
            y[:, 4:] = rng.uniform(0, 1, (n, nc, A_k))
            call.append(y)
        ys.append(call)
    if name == "a":
        for k, (A_k, b) in enumerate(bs):
            edge = boundary_boxes(b)
            for c, r in ((0, 0), (0, 2), (1, 0)):
                ys[c][k][r, :4, b[0]:b[0] + N_EDGE] = edge
    return ys, calls_rows(), [b for _, b in bs], A_tot


def launches(ys, rows, branches):
    """The K launches of every call, in order: (call, k, y_k, rows, branch)."""
    return [(c, k, ys[c][k], rows[c], branches[k]) for c in range(len(ys)) for k in range(len(branches))]


def edge_outcomes(merged, ys, branches, A_tot, nc_row=4):
    """Per branch, ``cut[margin][side][t]`` (bool) of the planted boxes in slot (frame 0, slot 0), every edge interior:
    a planted box counts as cut when its first score came out 0 although it went in non-zero."""
    res = []
    for k, b in enumerate(branches):
        got = merged[0, nc_row, b[2]:b[2] + N_EDGE]
        went_in = ys[0][k][0, nc_row, b[0]:b[0] + N_EDGE]
        assert (went_in > 0).all()
        assert ((got == 0) | (got == went_in)).all()
        res.append((got == 0).reshape(len(MARGINS), len(SIDES), 3))
    return res


def assert_each_outcome_occurs(cut, cut_margin):
    """``cut`` = one branch's entry of :func:`edge_outcomes`. On the boundary: cut (<= and >= include it); one step to
    the margin's side of it: cut; one step to the other side: kept. Low sides (left, top) are cut below the boundary,
    high sides (right, bottom) above it."""
    if cut_margin is None:
        assert not cut.any()
        return
    mi = MARGINS.index(float(cut_margin))
    for si, side in enumerate(SIDES):
        on, below, above = cut[mi, si]
        assert on, (side, "on the boundary")
        if side in ("left", "top"):
            assert below and not above, side
        else:
            assert above and not below, side
