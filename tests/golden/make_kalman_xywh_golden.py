"""Records tests/golden/kalman_xywh.npz from the reference's KalmanFilterXYWH. Run by hand:

    python tests/golden/make_kalman_xywh_golden.py <reference checkout>

As make_kalman_golden.py: the reference's ``ultralytics/trackers/utils/kalman_filter.py`` imports only numpy and scipy
and is loaded from its file path, never through the ``ultralytics.trackers`` package (whose ``__init__`` pulls in
``matching`` and with it ``lap``). Recorded, for 20 seeded tracks: ``initiate`` on an fp32 (cx, cy, w, h) measurement,
then predict / update / predict / update on the fp64 state, and ``multi_predict`` on the stacked states. ``initiate``'s
dtypes are recorded as the reference gives them (``init_mean_dtype``, ``init_cov_dtype``); the arrays are stored
promoted to fp64, which is exact. Recorded data only.

Also prints, and stores as ``max_rel_diff``, the largest relative difference between these results and
``yolosod_amd.utils.botsort``'s kf_initiate_xywh / kf_predict_xywh / kf_update_xywh (both fp64; only the summation
order differs): the Kalman pin of tests/test_botsort_cpu.py (1e-12) takes its margin over that value.
"""
import importlib.util
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))


def main(ref):
    path = Path(ref) / "ultralytics" / "trackers" / "utils" / "kalman_filter.py"
    spec = importlib.util.spec_from_file_location("_ref_kalman_filter", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    kf = mod.KalmanFilterXYWH()
    import yolosod_import  # noqa: F401
    from yolosod_amd.utils import botsort as bs

    rng = np.random.default_rng(35)
    n = 20
    z = np.zeros((3, n, 4), dtype=np.float32)  # the measurements of the three steps
    rec = {k: [] for k in ("init_mean", "init_cov", "pred1_mean", "pred1_cov", "upd1_mean", "upd1_cov", "pred2_mean",
                           "pred2_cov", "upd2_mean", "upd2_cov")}
    worst = 0.0
    dtypes = None

    def rel(a, b):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        return float((np.abs(a - b) / np.maximum(np.abs(b).max(), 1e-300)).max())

    for i in range(n):
        base = np.array([rng.uniform(0, 1920), rng.uniform(0, 1080), rng.uniform(8, 300), rng.uniform(8, 400)])
        for k in range(3):
            z[k, i] = (base + k * np.array([rng.uniform(-6, 6), rng.uniform(-6, 6), rng.uniform(-4, 4),
                                            rng.uniform(-4, 4)])).astype(np.float32)
        m, c = kf.initiate(z[0, i])
        dtypes = (str(np.asarray(m).dtype), str(np.asarray(c).dtype))
        m = np.asarray(m, dtype=np.float64)  # the definition keeps the state in fp64 from the start
        c = np.asarray(c, dtype=np.float64)
        mm, cc = bs.kf_initiate_xywh(z[0, i])
        worst = max(worst, rel(mm, m), rel(cc, c))
        rec["init_mean"].append(m), rec["init_cov"].append(c)
        for step, k in (("pred1", None), ("upd1", 1), ("pred2", None), ("upd2", 2)):
            if k is None:
                m, c = kf.predict(m, c)
                mm, cc = bs.kf_predict_xywh(mm, cc)
            else:
                m, c = kf.update(m, c, z[k, i])
                mm, cc = bs.kf_update_xywh(mm, cc, z[k, i])
            worst = max(worst, rel(mm, m), rel(cc, c))
            rec[step + "_mean"].append(np.asarray(m, dtype=np.float64))
            rec[step + "_cov"].append(np.asarray(c, dtype=np.float64))
            mm, cc = np.asarray(m, dtype=np.float64).copy(), np.asarray(c, dtype=np.float64).copy()  # no drift
    out = {k: np.stack(v) for k, v in rec.items()}
    mp_mean, mp_cov = kf.multi_predict(out["upd2_mean"].copy(), out["upd2_cov"].copy())
    for i in range(n):
        mm, cc = bs.kf_predict_xywh(out["upd2_mean"][i], out["upd2_cov"][i])
        worst = max(worst, rel(mm, mp_mean[i]), rel(cc, mp_cov[i]))
    out.update(z=z, multi_mean=np.asarray(mp_mean, dtype=np.float64), multi_cov=np.asarray(mp_cov, dtype=np.float64),
               max_rel_diff=np.float64(worst), init_mean_dtype=np.array(dtypes[0]), init_cov_dtype=np.array(dtypes[1]),
               numpy_version=np.array(np.__version__))
    dst = Path(__file__).resolve().parent / "kalman_xywh.npz"
    np.savez_compressed(dst, **out)
    print(f"{dst.name}: {n} tracks, initiate gives mean {dtypes[0]} / cov {dtypes[1]} (numpy {np.__version__}), "
          f"largest relative difference to utils.botsort {worst:.3e}")


if __name__ == "__main__":
    main(sys.argv[1])
