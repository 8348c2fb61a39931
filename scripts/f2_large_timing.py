"""Cost of the large-frame kernel alone (k_f2_large, csrc/lmx_f2.hip) at 2049, 4096, 8192 and 16384 records in one frame: records on a
lattice with few similarities and templates (many ties, bins of hundreds), through lmx_debug_device_finalize_cluster_large, against the
host path on the same records (lmx_merge_raw: insertion order + std::sort + std::unique, then lmx_cluster_matches).  The hook's wall time
includes its allocations and copies; run under `rocprofv3 --kernel-trace --stats` for the kernel's own duration (one launch per size and
repeat, in the order of the sizes).  Results are compared first.  Needs a GPU.
usage: f2_large_timing.py [repeats]"""
import sys, time
sys.path.insert(0, ".")
import numpy as np
from linemod_pose_estimation_amd import RAW_MATCH_DTYPE
from linemod_pose_estimation_amd.detector import cluster_matches, debug_device_finalize_cluster_large, merge_raw

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
rng = np.random.default_rng(1)
n_t = 12
dists = 0.5 + 0.1 * (np.arange(n_t) % 3)
rects = np.stack([np.zeros(n_t), np.zeros(n_t), rng.integers(8, 60, n_t), rng.integers(8, 60, n_t)], 1).astype(np.int32)
side = (dists, rects, 10, 0.5, 0.1, 2)
for n in (2049, 4096, 8192, 16384):
    r = np.zeros(n, RAW_MATCH_DTYPE)
    r["x"] = 60 * rng.integers(0, 4, n) + rng.integers(0, 3, n)
    r["y"] = 60 * rng.integers(0, 3, n) + rng.integers(0, 3, n)
    r["similarity"] = rng.choice(np.asarray([91.25, 85.5, 80.0], np.float32), n)
    r["template_id"] = rng.integers(0, n_t, n)
    r["order_key"] = rng.permutation(n).astype(np.uint64) * np.uint64(977) + np.uint64(1 << 33)
    t_dev, t_host = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        (m, c, mem, status), = debug_device_finalize_cluster_large(r, 1, *side)
        t1 = time.perf_counter()
        hm = merge_raw(r, cap=n)
        hc, hmem = cluster_matches(hm, *side)
        t2 = time.perf_counter()
        t_dev.append(t1 - t0)
        t_host.append(t2 - t1)
        assert status == 0 and m.tobytes() == hm.tobytes() and len(c) == len(hc) and c["score"].tobytes() == hc["score"].tobytes()
        assert np.array_equal(mem, hmem[:len(mem)])
    print("%5d records: %5d final matches, %3d clusters | hook with the large kernel (allocations and copies included) %.3f ms, host path %.3f ms (medians of %d)"
          % (n, len(m), len(c), 1e3 * np.median(t_dev), 1e3 * np.median(t_host), reps), flush=True)
