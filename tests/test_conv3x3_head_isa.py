"""CPU: the tower conv with the head's tail (csrc/conv3x3.hip, conv3x3_head_kernel) in the gfx950 code object (hipcc -S,
no GPU): the six instances (three geometries x box / class) use no scratch, at most 256 VGPRs and at most 81,920 B of
LDS, so that two workgroups per CU stay resident as for the plain conv; and the bank enumeration of the fp32 feature
tile between the conv and the tail. Only the kernel descriptors' metadata is read."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "yolo-sod_amd" / "csrc"
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)

MAX_VGPRS = 256
MAX_LDS = 81920   # two workgroups in a CU's 160 KiB
HT_RS = 68        # the feature tile's row stride in floats (conv3x3.hip)


def _descriptors(tmp_path):
    out = tmp_path / "conv3x3.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", f"-I{CSRC}",
                    "-o", str(out), str(CSRC / "conv3x3.hip")], check=True, capture_output=True, timeout=600)
    text = out.read_text()
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)", text):
        desc = text[m.start():text.find(".end_amdhsa_kernel", m.start())]
        res[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+)\s+(\d+)\s*$", desc, re.M)}
    return res


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_head_kernel_resources(tmp_path):
    ds = {n: d for n, d in _descriptors(tmp_path).items() if "conv3x3_head_kernel" in n}
    assert len(ds) == 6, sorted(ds)
    for name, d in sorted(ds.items()):
        print(f"{name}: {d['next_free_vgpr']} VGPRs, LDS {d['group_segment_fixed_size']}, "
              f"scratch {d['private_segment_fixed_size']}")
        assert d["private_segment_fixed_size"] == 0, name
        assert d["next_free_vgpr"] <= MAX_VGPRS, name
        assert 256 * HT_RS * 4 + 2048 <= d["group_segment_fixed_size"] <= MAX_LDS, name


def test_source_states_the_row_stride():
    assert f"constexpr int HT_RS = {HT_RS};" in (CSRC / "conv3x3.hip").read_text()


def _col(c, px):
    return c ^ ((px & 8) >> 2)


def test_feature_tile_is_free_of_bank_conflicts():
    """4-byte LDS writes and reads are served per 32-lane half with banks of 4 bytes mod 32. The conv's lane (g, l15)
    writes channel cb 16 + l15 of pixels 4 g + e of a block; the tail's lane (g, j) reads channel g + 4 q of pixel j."""
    for half in (0, 1):
        lanes = range(32 * half, 32 * half + 32)
        for blk in (0, 5, 15):
            for cb in range(4):
                for e in range(4):
                    banks = {((blk * 16 + 4 * (ln >> 4) + e) * HT_RS + _col(16 * cb + (ln & 15), 4 * (ln >> 4) + e)) % 32
                             for ln in lanes}
                    assert len(banks) == 32, ("write", half, blk, cb, e)
            for q in range(16):
                banks = {((blk * 16 + (ln & 15)) * HT_RS + _col((ln >> 4) + 4 * q, ln & 15)) % 32 for ln in lanes}
                assert len(banks) == 32, ("read", half, blk, q)


def test_feature_tile_addresses_round_trip():
    """Every (pixel, channel) of a block has one address, and the tail reads what the conv wrote."""
    seen = {}
    for px in range(16):
        for c in range(64):
            a = px * HT_RS + _col(c, px)
            assert a not in seen and _col(c, px) < 64
            seen[a] = (px, c)
    assert len(seen) == 16 * 64
