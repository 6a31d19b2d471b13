import os
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(GOLDEN))

# bench.py (imported by tests/test_bench_cli.py at collection) points MIOpen's user find-db at the tracked
# yolo-sod_amd/miopen_db, and MIOpen appends the solvers it finds for the tests' conv shapes to that file. The suite
# works on a throw-away copy instead: same recorded solvers, and the tracked file stays as committed.
if "MIOPEN_USER_DB_PATH" not in os.environ:
    import atexit
    import shutil
    import tempfile
    _db = tempfile.mkdtemp(prefix="yolosod_miopen_db_")
    for _f in (ROOT / "yolo-sod_amd" / "miopen_db").glob("*.ufdb.txt"):
        shutil.copy2(_f, _db)
    os.environ["MIOPEN_USER_DB_PATH"] = _db
    atexit.register(shutil.rmtree, _db, ignore_errors=True)

import yolosod_import  # noqa: E402,F401  (registers the yolosod_amd package)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (runs the HIP kernels)")


def golden(name: str):
    return np.load(GOLDEN / f"{name}.npz", allow_pickle=False)


@pytest.fixture(scope="session")
def cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")
