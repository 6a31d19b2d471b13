"""CPU: what the compiler made of the merge-NMS kernel (hipcc -S for gfx950, no GPU): it uses no scratch (the eight
kept rows' fp64 partial sums stay in registers) and its sums are fp64."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "yolo-sod_amd" / "csrc"
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_nms_merge_kernel_has_no_scratch_and_sums_in_fp64(tmp_path):
    out = tmp_path / "nms.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only",
                    "-S", f"-I{CSRC}", f"-I{ROOT / 'include'}", "-o", str(out), str(CSRC / "nms.hip")], check=True,
                   capture_output=True, timeout=600)
    text = out.read_text()
    names = [m.group(1) for m in re.finditer(r"^(_Z[^:\s]*nms_merge_kernel[^:\s]*):", text, re.M)]
    assert len(names) == 1, names
    name = names[0]
    start = text.index(name + ":")
    body = text[start:text.index("s_endpgm", start)]
    assert re.search(r"v_(add|fma)_f64", body), "no fp64 accumulation in the merge kernel"
    meta = re.search(r"\.name:\s+" + re.escape(name) + r"\n\s+\.private_segment_fixed_size:\s*(\d+)", text)
    assert meta and int(meta.group(1)) == 0, meta and meta.group(0)
