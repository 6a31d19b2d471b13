"""CPU: the LDS layout of the tiled stride-2 3x3 conv kernel's pixel planes (csrc/conv3x3s2.hip, conv3x3s2_t2_kernel) is
conflict-free for every block shape and every tap.

A lane (g, l15) of a pixel fragment reads 16 bytes at byte (pixel * PS + 8 g) * 2 of a plane; for tap (ty, tx) its
pixel is (2 (l15 / BW) + ty) * RS + 2 (l15 % BW) + tx of the block's origin (blocks of BW x 16 / BW output pixels, input
pixels two apart). gfx950 serves a ds_read_b128 in four groups of 16 lanes - {0-3, 12-15, 20-27}, {4-11, 16-19,
28-31} and the same + 32 - one LDS cycle per group when the group's sixteen 16-byte slots fall into sixteen
different 16-byte columns of the 256-byte bank row. This enumerates the groups for the three geometries' (BW, RS) at
PS = 40 halves, read back from the source so the table cannot drift, and shows that the bare halo widths of the
40 x 2 and 20 x 4 tiles (81 and 41 pixels) would conflict."""
import re
from pathlib import Path

SRC = Path(__file__).resolve().parents[1] / "yolo-sod_amd" / "csrc" / "conv3x3s2.hip"
GROUPS = [[*range(0, 4), *range(12, 16), *range(20, 28)], [*range(4, 12), *range(16, 20), *range(28, 32)]]
GROUPS += [[lane + 32 for lane in grp] for grp in GROUPS]


def worst_way(bw, rs, ps, tap=(0, 0), origin=0):
    """The largest number of distinct addresses on one 16-byte bank column within a lane group (1 = conflict-free)."""
    worst = 0
    for grp in GROUPS:
        cols = {}
        for lane in grp:
            g, l15 = lane >> 4, lane & 15
            px = origin + (2 * (l15 // bw) + tap[0]) * rs + 2 * (l15 % bw) + tap[1]
            addr = px * ps * 2 + 16 * g
            cols.setdefault((addr // 16) % 16, set()).add(addr)
        worst = max(worst, max(len(a) for a in cols.values()))
    return worst


def worst_over_taps(bw, rs, ps, tbx=1, tby=1):
    bh = 16 // bw
    return max(worst_way(bw, rs, ps, (ty, tx), 2 * by * bh * rs + 2 * bx * bw)
               for ty in range(3) for tx in range(3) for by in range(tby) for bx in range(tbx))


def _geometries():
    text = SRC.read_text()
    a, b = map(int, re.search(r"constexpr int PS = (\d+) \+ (\d+);", text).groups())
    geos = re.findall(r"static constexpr int BW = (\d+), TBX = (\d+), TBY = (\d+), RS = (\d+);", text)
    return a + b, [tuple(map(int, g)) for g in geos]


def test_every_geometry_reads_conflict_free():
    ps, geos = _geometries()
    assert ps == 40 and len(geos) == 3
    assert [(bw, tbx, tby) for bw, tbx, tby, _ in geos] == [(16, 2, 2), (8, 5, 1), (4, 5, 1)]
    for bw, tbx, tby, rs in geos:
        bh = 16 // bw
        hc, hr = 2 * tbx * bw + 1, 2 * tby * bh + 1
        assert rs >= hc  # the LDS row holds the halo row
        assert hr * hc * 8 <= 32 * 256  # staged items per thread: one in-image bit each
        # two planes + the bias / gate arrays: two workgroups per CU within 160 KB
        assert 2 * (2 * hr * rs * ps * 2 + 512 * 4 + 32 * 4 + hr * hc * 4) <= 160 * 1024
        assert worst_over_taps(bw, rs, ps, tbx, tby) == 1, (bw, rs)


def test_bare_halo_rows_would_conflict():
    assert worst_way(8, 81, 40) == 2  # 8 x 2 blocks on the 81-pixel halo row
    assert worst_way(4, 41, 40) == 2  # 4 x 4 blocks on the 41-pixel halo row
    # the smallest conflict-free row strides at or above the halo width are the ones the kernel uses, and they are
    # the residues the layout argument gives (a multiple of 8 for 8 x 2 blocks, 4 mod 8 for 4 x 4)
    ok8 = [rs for rs in range(81, 130) if worst_over_taps(8, rs, 40) == 1]
    ok4 = [rs for rs in range(41, 90) if worst_over_taps(4, rs, 40) == 1]
    assert ok8[0] == 88 and all(rs % 8 == 0 for rs in ok8)
    assert ok4[0] == 44 and all(rs % 8 == 4 for rs in ok4)
