"""CPU: resources of every conv1x1_x2_kernel instance (csrc/conv1x1x2.hip) from the kernel descriptors of a
hipcc -S build for gfx950, no GPU: no scratch, at most 256 VGPRs (two 256-thread workgroups per CU) and the LDS of
the form - one pair of staged planes (2 x 64 pixels x 272 B = 34816 B) or two (the double-buffered forms, DB = true in
the instance's name)."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "yolo-sod_amd" / "csrc"
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)
PLANES = 2 * 64 * (128 + 8) * 2  # bytes of one pair of planes


@pytest.fixture(scope="module")
def descriptors(tmp_path_factory):
    out = tmp_path_factory.mktemp("c1isa") / "conv1x1x2.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "--cuda-device-only", "-S", f"-I{CSRC}",
                    f"-I{ROOT / 'include'}", "-o", str(out), str(CSRC / "conv1x1x2.hip")], check=True,
                   capture_output=True, timeout=600)
    text = out.read_text()
    meta = text[text.index("amdhsa.kernels:"):]
    ks = {}
    for blk in re.split(r"\n  - (?=\.agpr_count:)", meta)[1:]:
        f = {k: v for k, v in re.findall(r"^\s*\.(\w+):\s+(\S+)$", blk, re.M)}
        if "conv1x1_x2_kernel" in f.get("name", ""):
            ks[f["name"]] = f
    return ks


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_every_instance_fits(descriptors):
    # <DUAL, 64, CPW, DB>: CPW 1 single-buffered only, CPW 2 and 4 in both forms, each with and without the dual store
    want = {(d, c, b) for d in (0, 1) for c, b in ((1, 0), (2, 0), (2, 1), (4, 0), (4, 1))}
    got = set()
    for name, f in descriptors.items():
        m = re.search(r"conv1x1_x2_kernelILb([01])ELi64ELi(\d)ELb([01])EE", name)
        assert m, name
        dual, cpw, db = (int(v) for v in m.groups())
        got.add((dual, cpw, db))
        assert int(f["private_segment_fixed_size"]) == 0, (name, f["private_segment_fixed_size"])
        assert int(f["vgpr_spill_count"]) == 0 and int(f["sgpr_spill_count"]) == 0, name
        assert int(f["vgpr_count"]) <= 256 and int(f["agpr_count"]) == 0, (name, f["vgpr_count"], f["agpr_count"])
        assert int(f["group_segment_fixed_size"]) == PLANES * (2 if db else 1), (name, f["group_segment_fixed_size"])
    assert got == want, got ^ want
