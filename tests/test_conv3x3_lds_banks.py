"""CPU: the LDS layout of the 3x3 conv kernel's pixel planes (csrc/conv3x3.hip) is conflict-free for every block shape.

A lane (g, l15) of a pixel fragment reads 16 bytes at byte (pixel(l15) * PS + 8 g) * 2 of a plane, pixel = row * RS +
column of the block's pixel l15 (blocks of BW x 16 / BW pixels). gfx950 serves a ds_read_b128 in four groups of 16
lanes - {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32 - one LDS cycle per group when the group's
sixteen 16-byte slots fall into sixteen different 16-byte columns of the 256-byte bank row. This enumerates the
groups for the three geometries' (BW, RS) at PS = 48 halves, reads them back from the source so the table cannot
drift, and shows the strides the small-map geometries would have had without padding do conflict."""
import re
from pathlib import Path

SRC = Path(__file__).resolve().parents[1] / "yolo-sod_amd" / "csrc" / "conv3x3.hip"
GROUPS = [[*range(0, 4), *range(12, 16), *range(20, 28)], [*range(4, 12), *range(16, 20), *range(28, 32)]]
GROUPS += [[lane + 32 for lane in grp] for grp in GROUPS]


def worst_way(bw, rs, ps):
    """The largest number of distinct addresses on one 16-byte bank column within a lane group (1 = conflict-free)."""
    worst = 0
    for grp in GROUPS:
        cols = {}
        for lane in grp:
            g, l15 = lane >> 4, lane & 15
            addr = ((l15 // bw) * rs + l15 % bw) * ps * 2 + 16 * g
            cols.setdefault((addr // 16) % 16, set()).add(addr)
        worst = max(worst, max(len(a) for a in cols.values()))
    return worst


def _geometries():
    text = SRC.read_text()
    ps = int(re.search(r"constexpr int PS = (\d+);", text).group(1))
    geos = re.findall(r"static constexpr int BW = (\d+), TBX = (\d+), TBY = (\d+), RS = (\d+);", text)
    return ps, [tuple(map(int, g)) for g in geos]


def test_every_geometry_reads_conflict_free():
    ps, geos = _geometries()
    assert ps == 48 and len(geos) == 3
    for bw, tbx, tby, rs in geos:
        assert rs >= tbx * bw + 2  # the LDS row holds the halo row
        assert tbx * tby <= 16
        assert (tby * (16 // bw) + 2) * (tbx * bw + 2) <= 340  # halo pixels: the staging registers stay as they are
        assert worst_way(bw, rs, ps) == 1, (bw, rs)
        # any tap shift moves every lane by the same number of pixels = a multiple of 96 bytes: the columns rotate
        # together (6 t mod 16), so one tap's result holds for all nine


def test_unpadded_small_map_rows_would_conflict():
    assert worst_way(4, 22, 48) == 2  # 4 x 4 blocks on the 22-pixel halo row
    assert worst_way(8, 42, 48) == 2  # 8 x 2 blocks on the 42-pixel halo row
    # the smallest conflict-free row strides at or above the halo width are the ones the kernel uses
    assert min(rs for rs in range(22, 64) if worst_way(4, rs, 48) == 1) == 28
    assert min(rs for rs in range(42, 96) if worst_way(8, rs, 48) == 1) == 48
