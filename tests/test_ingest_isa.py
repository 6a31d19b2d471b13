"""CPU: what the compiler made of the ingest kernels (hipcc -S for gfx950, no GPU). A workgroup belongs to one frame,
so the frame's descriptor is read with scalar loads and no load sits in a waterfall loop (tests/test_isa_guard.py);
the kernels use no scratch."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "yolo-sod_amd" / "csrc"
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_ingest_kernels_descriptor_loads_are_uniform_and_nothing_spills(tmp_path):
    out = tmp_path / "ingest.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "--cuda-device-only", "-S", f"-I{CSRC}", "-o", str(out),
                    str(CSRC / "ingest.hip")], check=True, capture_output=True, timeout=300)
    text = out.read_text()
    bodies = {}
    for m in re.finditer(r"^(_Z[^:\s]+):", text, re.M):
        bodies[m.group(1)] = text[m.end():text.find("s_endpgm", m.end())]
    ks = {k: v for k, v in bodies.items() if "letterbox_ingest_kernel" in k}
    assert len(ks) == 2, list(bodies)  # fp32 and bf16 output
    for name, body in ks.items():
        assert body.count("v_readfirstlane") <= 16, f"{name}: waterfall loads?"
        assert len(re.findall(r"s_load_dwordx\d+", body)) >= 2, f"{name}: descriptor not read with scalar loads"
    scratch = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert scratch and all(int(v) == 0 for v in scratch), scratch
