#!/usr/bin/env python3
"""bench.py -- per-patient nlml+gradient evaluations/s of the MI355X-native MedGP hot path.

Contract (driver):  python bench.py --gpus N --steps K --warmup W   (N > 1: launched by torch.distributed.run,
one rank per GPU).  Prints ONE JSON line on rank 0.

Workload (BASELINE.json metric "per-patient log-lik+grad evals/sec at D=24 N=512"): the per-GPU shard of
config 4 -- 512 synthetic patients x N=512 observations, D=24 outputs, Q=5, R=8 (H=1114 hypers), LMC-SM kernel,
Gaussian-MO likelihood, zero mean, hierarchical-gamma prior (mode 2), fp64.  One step = one nlml+gradient
evaluation of every patient of the shard (one theta each).  Weak scaling (default): every rank owns 512 patients.
--scaling strong: the FIXED 4096-patient cohort of BASELINE config 4 is LPT-partitioned over the ranks
(medgp_amd/shard.py; 4096 / N patients per rank), so the N = 1, 2, 4 lines are that cohort's own numbers.  Either way the
cohort is sharded with no data-path collective (patients are independent).  Inputs (patients, theta) are
resident in HBM before the timed region; outputs stay in HBM.

A plain run sets up, warms up, times --steps steps and prints the line; --dump-outputs DIR also writes the last timed step's results.
Everything beside the headline -- roofline and per-kernel split of the step, sustained rate, other_configs, CPU baseline -- runs
with --full only.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FP64_PEAK_TFLOPS = 78.6   # MI355X dense fp64 (vector = matrix) peak, AMD spec; see DESIGN.md section 5
HBM_PEAK_GBS = 8000.0     # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec


def alg_work(kernel, N, Q, D, H):
    """Algorithmic work of ONE patient in one launch of `kernel`.
    Returns (flop, bytes, bound)."""
    pairs = Q * N * (N + 1) / 2
    table = {
        "k_prep": (Q * D * D * 2 * 8 + 40.0 * Q * N, 8.0 * (H + 2 * Q * N), "hbm"),
        "k_assemble": (40.0 * pairs, 8.0 * N * N / 2, "mfma"),
        "k_lauum": (N ** 3 / 3.0 + 2.0 * N * N, 8.0 * N * N, "mfma"),
        "k_gradbins": (40.0 * pairs, 8.0 * N * N / 2, "mfma"),
        # fused Cholesky + triangular inverse + forward solve (potrf N^3/3 + trtri N^3/3 + 2 solves 2N^2);
        # bytes: read K lower (4N^2), write L lower + U upper (8N^2)
        "k_cholinv": (2.0 * N ** 3 / 3.0 + 4.0 * N * N, 12.0 * N * N, "mfma"),
        # fused W = U U^T - alpha alpha^T (N^3/3) + gradient block sums (40 flop-equivalents per pair);
        # bytes: read U upper once (4N^2)
        "k_wgrad": (N ** 3 / 3.0 + 2.0 * N * N + 40.0 * pairs, 4.0 * N * N, "mfma"),
        # multi-CU look-ahead schedule (few large patients): the same algorithmic work as k_cholinv, spread over N / 64 launches
        "k_la_step": (2.0 * N ** 3 / 3.0 + 4.0 * N * N, 12.0 * N * N, "mfma"),
        "k_epilogue": (2.0 * Q * D * D * 8 + 8.0 * H, 8.0 * (2 * H + 3 * Q * D * D), "hbm"),
    }
    return table.get(kernel, (0.0, 0.0, "hbm"))


def shape_traffic(label, kernel):
    """HBM bytes per launch of `kernel` on another measured shape (profiles/rNN_pmc_summary.json "_shapes", round 6), or None when the
    device sources have changed since the passes.  For k_la_step the per-call figure is the sum over its launches: mean x launches per call
    is formed by the caller."""
    import glob
    cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_pmc_summary.json")))
    if not cands:
        return None
    try:
        d = json.load(open(cands[-1]))
    except (OSError, ValueError):
        return None
    if d.get("_meta", {}).get("csrc_sha256") != csrc_digest():
        return None
    e = next((v for k, v in d.get("_shapes", {}).get(label, {}).items() if k.split("<")[0] == kernel), None)
    if not e or "write_bytes" not in e:
        return None
    return e["fetch_bytes_x2_if_wide_loads"] + e["write_bytes"]


def leg_roofline(kernel_ms, N, Q, D, H, P, nlml_only=False, shape=None, launches=1):
    """Roofline fraction of the DOMINANT kernel of an auxiliary leg (verdict r5 item 6): its algorithmic flops (alg_work x the P
    entries of the call; nlml only: no inverse, N^3/3 + 2 N^2 per entry) / its HIP-event time per call / fp64 peak.  For the
    look-ahead schedule the time is the sum over the N / 64 launches of k_la_step."""
    if not kernel_ms:
        return None
    dom = max(kernel_ms, key=kernel_ms.get)
    flop, byts, bound = alg_work(dom, N, Q, D, H)
    if nlml_only and dom in ("k_cholinv", "k_la_step"):
        flop, byts = N ** 3 / 3.0 + 2.0 * N * N, 8.0 * N * N
    ms = kernel_ms[dom]
    if bound == "mfma":
        ach = flop * P / (ms * 1e-3) / 1e12
        r = {"kernel": dom, "ms_per_call": ms, "bound": "mfma", "achieved": ach, "unit": "TFLOP/s", "frac": ach / FP64_PEAK_TFLOPS}
        tr = shape_traffic(shape, {"k_la_step": "k_la_step", "k_cholinv": "k_cholinv"}.get(dom, dom)) if shape else None
        if tr:
            tr *= launches      # (bytes per launch x launches of this kernel per call)
            r.update({"traffic": tr, "hbm_frac": tr / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "traffic_ratio": tr / (byts * P)})
        return r
    ach = byts * P / (ms * 1e-3) / 1e9
    return {"kernel": dom, "ms_per_call": ms, "bound": "hbm", "achieved": ach, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS}


def csrc_digest():
    """sha256 over the device sources (medgp_amd/csrc/*.h, *.hip): identifies the kernels a PMC summary was taken from."""
    import glob
    import hashlib
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(ROOT, "medgp_amd", "csrc", "*.h")) + glob.glob(os.path.join(ROOT, "medgp_amd", "csrc", "*.hip"))):
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()


def pmc_traffic(kernel, P, N):
    """HBM bytes per launch of `kernel` from the committed rocprofv3 PMC passes (profiles/rNN_pmc_summary.json, latest round: separate
    --pmc FETCH_SIZE / --pmc WRITE_SIZE runs of this same command; bytes = counter x 1024, FETCH_SIZE doubled for
    16-byte-per-lane streams as MI355X_MICROARCH.md's HBM section prescribes).  PMC and kernel-trace cannot be combined in
    one run, so the value is measured offline.  It is returned only for the shape it was measured on AND only while the
    device sources are byte-identical to the ones it was measured from (the summary records their digest and the git
    commit); otherwise null -- a stale number is worse than none.  Returns (bytes or None, provenance dict)."""
    import glob
    cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_pmc_summary.json")))   # the latest round's passes
    name = os.path.basename(cands[-1]) if cands else "r03_pmc_summary.json"
    prov = {"file": "profiles/" + name}
    try:
        d = json.load(open(os.path.join(ROOT, "profiles", name)))
    except (OSError, ValueError):
        return None, dict(prov, status="no PMC summary")
    meta = d.get("_meta", {})
    prov.update({"git_commit": meta.get("git_commit"), "csrc_sha256": (meta.get("csrc_sha256") or "")[:16]})
    if meta.get("csrc_sha256") != csrc_digest():
        return None, dict(prov, status="stale: device sources changed since the PMC passes")
    if (P, N) != (512, 512):
        return None, dict(prov, status="not measured for this shape")
    for name, v in d.items():
        if name.split("<")[0] == kernel and "derived" in v:
            return v["derived"]["fetch_bytes_x2_if_wide_loads"] + v["derived"]["write_bytes"], dict(prov, status="current")
    return None, dict(prov, status="kernel not in the summary")


def step_roofline(prof, prof_all, n_split, N, Q, D, H, P):
    """Roofline of the dominant kernel of the timed step (`--full`): its algorithmic work (alg_work) over its live HIP-event launch time,
    the HBM side from the committed PMC passes, and the per-kernel split of a step from `n_split` untimed steps."""
    # dominant kernel + roofline from the live HIP-event timings
    tot = {k: v[0] for k, v in prof.items() if v[1] > 0}
    dom = max(tot, key=tot.get)
    avg_ms = prof[dom][0] / prof[dom][1]
    flop, byts, bound = alg_work(dom, N, Q, D, H)
    if bound == "mfma":
        achieved = flop * P / (avg_ms * 1e-3) / 1e12
        roof = {"bound": "mfma", "achieved": achieved, "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s",
                "frac": achieved / FP64_PEAK_TFLOPS}
    else:
        achieved = byts * P / (avg_ms * 1e-3) / 1e9
        roof = {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS}
    traffic, traffic_prov = pmc_traffic(dom, P, N)
    # the HBM side of the same kernel (verdict r5 item 6): measured traffic / launch time against the 8 TB/s spec, and against the
    # algorithmic bytes (ratio > 1 = re-reads: the left-looking history of k_cholinv)
    roof.update({"hbm_frac": (traffic / (avg_ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if traffic else None,
                 "hbm_achieved_GBs": (traffic / (avg_ms * 1e-3) / 1e9) if traffic else None,
                 "traffic_ratio": (traffic / (byts * P)) if traffic and byts else None})
    roof.update({"traffic": traffic, "traffic_provenance": traffic_prov, "kernel": dom, "avg_launch_ms": avg_ms,
                 "alg_per_patient": {"flop": flop, "bytes": byts},
                 "kernel_ms_per_step": {k: round(v[0] / n_split, 4) for k, v in prof_all.items() if v[1] > 0},
                 "kernel_ms_per_step_source": "%d untimed steps behind the timed region, events around every launch; avg_launch_ms: live over the timed region" % n_split})
    return roof


def check_ranks(seen, world, backend):
    """None, or what is wrong with the set of ranks that took part: under nccl (one rank per GPU) the (host, uuid) pairs must be
    pairwise distinct and every rank must have reported."""
    if len(seen) != world or any(r is None for r in seen):
        return f"{sum(r is not None for r in seen)} of {world} ranks reported"
    if sorted(r["rank"] for r in seen) != list(range(world)):
        return "rank ids are not 0 .. %d: %s" % (world - 1, [r["rank"] for r in seen])
    if backend == "nccl":
        ids = [(r["host"], r["uuid"] or f"device{r['device']}") for r in seen]
        if len(set(ids)) != world:
            return "ranks share a GPU under the nccl backend: " + ", ".join(f"rank {r['rank']} -> {r['host']}:{r['device']} ({r['uuid']})" for r in seen)
    return None


def aggregate_time(t_local, world):
    """max over ranks of the local wall time (the driver's contract)."""
    import torch
    import torch.distributed as dist
    if world <= 1 and not (dist.is_available() and dist.is_initialized()):
        return float(t_local)
    if dist.get_backend() == "nccl":
        tt = torch.tensor([t_local], dtype=torch.float64, device="cuda")
    else:
        tt = torch.tensor([t_local], dtype=torch.float64)
    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    return float(tt.item())


def result_line(value, n_gpus, steps, warmup, ms_per_step, workload, extra, scaling="weak"):
    line = {
        "metric": "per-patient nlml+grad evals/sec at D=24 N=512",
        "value": value,
        "unit": "evals/s",
        "n_gpus": n_gpus,
        "steps": steps,
        "warmup": warmup,
        "ms_per_step": ms_per_step,
        "higher_is_better": True,
        "scaling": scaling,
        "vs_baseline": None,   # BASELINE.md holds no published number for this metric
        "dtype": "f64",
        "data": "synthetic",
        "config": {"workload": workload},
    }
    line.update(extra)
    return line


DUMP_LIMIT_BYTES = 64 * 10 ** 6   # --dump-outputs: at most this much in all


def dump_outputs(out_dir, gids, arrays, suffix="", limit=DUMP_LIMIT_BYTES):
    """--dump-outputs: `arrays` (name -> one row per patient: what a caller of the timed path receives) as out_dir/<name><suffix>.npy
    in float64, beside the patients' global ids (patient_ids<suffix>.npy).  When the rows would exceed `limit` bytes in all, a fixed
    sample of the patients (seed 0, the same for the same arguments) is written instead, in patient order."""
    os.makedirs(out_dir, exist_ok=True)
    n = len(gids)
    arrays = dict(arrays, patient_ids=np.asarray(gids))
    row_bytes = 8 * sum(int(np.prod(np.shape(a)[1:])) for a in arrays.values())
    rows = np.arange(n)
    budget = limit - 128 * len(arrays)        # (the .npy header of each file)
    if row_bytes * n > budget:
        rows = np.sort(np.random.default_rng(0).choice(n, size=max(1, budget // row_bytes), replace=False))
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, f"{name}{suffix}.npy"), np.asarray(a, dtype=np.float64)[rows])


def usable_cores():
    """Host cores this process may actually use: affinity mask capped by the cgroup CPU quota."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(float(txt[0]) / float(txt[1]))))
            else:
                q = int(txt[0])
                if q > 0:
                    per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                    n = min(n, max(1, q // per))
        except (OSError, ValueError, IndexError):
            pass
    return max(1, min(n, 64))


def cpu_baseline(D, N, Q, R, seed, budget_s=10.0):
    """The oracle ("port" of the reference's algorithm, per-hyper gradient loop as
    c_kernel_LMC_SM.cpp:222-325) timed on this box's host cores on a bounded sample of the same workload."""
    from medgp_amd import synth
    from oracle import oracle as O
    cores = usable_cores()
    pr = O.Prior.hier_gamma(Q, D, R, 0.01, 0.01)
    n_eval, t0 = 0, time.perf_counter()
    while True:
        m, t, y = synth.patient(seed, n_eval, D, N)
        th = synth.theta(seed, n_eval, 7, Q, D, R)
        r = O.nlml_grad(7, Q, D, R, m, t, y, th, flag_grad=True, grad_mode=O.GRAD_PER_HYPER, nthreads=cores, prior=pr)
        assert r["ok"]
        n_eval += 1
        el = time.perf_counter() - t0
        if el >= budget_s:
            break
        if n_eval >= 64:
            break
    return {"value": n_eval / el, "unit": "evals/s", "cores": cores, "kind": "port",
            "sample": f"{n_eval} patients of the same synthetic cohort (D={D}, N={N}, Q={Q}, R={R}), nlml+grad, "
                      f"oracle per-hyper gradient loop, OpenMP over hypers, {el:.1f} s"}


def other_configs(dev_index, seed, reps=5):
    """Short measurements of BASELINE configs 2, 3 and 5 on this GPU (outside the timed region of the headline; rank 0 at
    N = 1 only).  Whole evaluations (nlml + gradient, host-pointer API, wall clock incl. the theta / result transfers);
    `frac_fp64_peak` = F_alg x evaluations/s / 78.6 TFLOP/s with F_alg = N^3 + 6 N^2 + 80 Q N (N + 1) / 2."""
    import medgp_amd
    from medgp_amd import synth
    out = {}
    shapes = [
        ("config2_256xN256_D2", 2, 256, 5, 2, 256, 0.0, False),
        ("config3_1xN2048_D24", 24, 2048, 5, 8, 1, 0.0, False),
        ("config3_batched_16xN2048_D24", 24, 2048, 5, 8, 16, 0.0, False),
        ("config5_1xN4096_D64_sparse_prior2", 64, 4096, 5, 8, 1, 0.5, True),
    ]
    def guarded(name, fn):
        """An auxiliary measurement must never cost the headline line: record the failure instead (advisor finding, round 2)."""
        try:
            fn()
        except Exception as e:   # noqa: BLE001
            out[name] = {"error": f"{type(e).__name__}: {e}"[:300]}

    def one_shape(name, D, N, Q, R, P, sparse, prior):
        H = synth.num_hyp(7, Q, D, R)
        ctx = medgp_amd.Context(7, Q, D, R, device=dev_index)
        ctx.reserve(P, N, P)
        nu = P if P * N <= 65536 else min(P, 8)   # distinct patients (a replicated cohort hides 3-5 % in L2 hits)
        pts = [synth.patient(seed + 1, p, D, N) for p in range(nu)]
        ths = [synth.theta(seed + 1, p, 7, Q, D, R, sparse_frac=sparse) for p in range(nu)]
        ctx.set_patients(np.arange(P), [pts[s % nu] for s in range(P)])
        th = np.stack([ths[s % nu] for s in range(P)])
        if prior:
            f, ty, ex, p0, p1 = synth.hier_gamma_prior(Q, D, R, 0.01)
            ty = ty.copy()
            ty[np.where(ths[0] == 0.0)[0]] = 0      # test-time clamp of the exactly-zero A entries (ref: c_prior.cpp:118-140)
            ctx.set_prior(-1, f, ty, ex, p0, p1)
        slots = np.arange(P)
        nl, g, st = ctx.nlml_grad(slots, th, True)
        assert np.all(st >= 0) and np.all(np.isfinite(nl)), name
        ctx.nlml_grad(slots, th, True)
        t0 = time.perf_counter()
        for _ in range(reps):
            ctx.nlml_grad(slots, th, True)
        dt = (time.perf_counter() - t0) / reps
        ctx.profile_reset()
        ctx.profile_enable(True)
        ctx.nlml_grad(slots, th, True)
        prof = {k: round(v[0], 4) for k, v in ctx.profile_read().items() if v[1] > 0}
        ctx.profile_enable(False)
        f_alg = N ** 3 + 6 * N * N + 80 * Q * N * (N + 1) / 2
        out[name] = {"patients": P, "N": N, "D": D, "Q": Q, "R": R, "H": H, "ms_per_call": 1e3 * dt, "evals_per_s": P / dt,
                     "frac_fp64_peak": f_alg * P / dt / 1e12 / FP64_PEAK_TFLOPS, "kernel_ms": prof,
                     "dominant_kernel": leg_roofline(prof, N, Q, D, H, P, shape="config3_1xN2048" if name == "config3_1xN2048_D24" else None,
                                                     launches=N // 64 if name == "config3_1xN2048_D24" else 1)}
        ctx.close()

    for shp in shapes:
        guarded(shp[0], lambda shp=shp: one_shape(*shp))
    guarded("config3_patient_inside_a_lockstep_batch", lambda: config3_in_batch(out, dev_index, seed, reps))
    guarded("screening_1000xN512_D24_nlml_only", lambda: screening(out, dev_index, seed, reps))
    guarded("config4_full_4096xN512_D24", lambda: config4_full(out, dev_index, seed))
    guarded("cohort_mode_kde_P4096_D24_one_cluster", lambda: cohort_kde(out, dev_index, seed))
    guarded("host_paths", lambda: host_paths(out, dev_index, seed))
    guarded("ragged_cohort_300_lognormal_D24", lambda: ragged_cohort(out, dev_index, seed))
    return out


def ragged_cohort(out, dev_index, seed, reps=5):
    """A heavy-tailed cohort in ONE call (round 5): 300 patients, log-normal sizes (synth.ragged_sizes: median ~260, the largest
    5832 observations), D = 24, hier-gamma prior, nlml + gradient through the host-pointer API.  `after` = the library's default
    plan (size classes with their own leading dimension, launch geometry and factorisation route, on separate streams);
    `one_stream` = the same classes back to back; `before` = rounds 1-4 (MEDGP_NO_CLASSES=1: one route for the whole call chosen from
    its entry count).  frac_fp64_peak = sum_p F_alg(N_p) / time / 78.6 TFLOP/s.  Reference for the behaviour: the job generator buckets
    patients by size (ref: scripts/slurm_della.json:6-62, medgpc/util/run_exp_generator.py:213-260)."""
    import medgp_amd
    from medgp_amd import synth
    P, D, Q, R = 300, 24, 5, 8
    pts, th, ns = synth.ragged_cohort(0, P, D, 7, Q, R)
    f_alg = float(sum(n ** 3 + 6 * n ** 2 + 80 * Q * n * (n + 1) / 2 for n in ns.astype(np.float64)))
    slots = np.arange(P)
    res = {}
    saved = {k: os.environ.get(k) for k in ("MEDGP_CLASS_STREAMS", "MEDGP_NO_CLASSES", "MEDGP_MEM_BUDGET_GB")}
    try:
        variants = [("after", {}, reps), ("one_stream", {"MEDGP_CLASS_STREAMS": "0"}, reps)]
        if os.environ.get("MEDGP_BENCH_RAGGED_BEFORE"):
            # rounds 1-4 behaviour, on request only: it needs 2 x 83 GB of per-entry matrices (300 entries at the leading dimension of the
            # largest), and memory a process has used is wiped by the driver before the next process gets it -- every run started behind
            # this leg (the driver's N = 2, 4, 8 runs; a user's trainer) then waits seconds for its allocations (scratch/alloc_dirty.hip)
            variants.append(("before", {"MEDGP_NO_CLASSES": "1", "MEDGP_MEM_BUDGET_GB": "200"}, 1))
        for name, env, r in variants:
            for k in saved:
                os.environ.pop(k, None)
            os.environ.update(env)
            ctx = medgp_amd.Context(7, Q, D, R, device=dev_index)     # (the switches are read at creation)
            ctx.reserve(P, int(ns.max()), P)
            if name != "before":
                ctx.reserve_plan(ns)          # the per-entry buffers sized once from the sizes (5.5 GB; the capacities alone would ask for 2 x 83 GB)
            ctx.set_patients(slots, pts)
            ctx.set_prior(-1, *synth.hier_gamma_prior(Q, D, R, 0.01))
            nl, g, st = ctx.nlml_grad(slots, th, True)
            assert np.all(st >= 0) and np.all(np.isfinite(nl)), name
            t0 = time.perf_counter()
            for _ in range(r):
                ctx.nlml_grad(slots, th, True)
            dt = (time.perf_counter() - t0) / r
            res[name] = {"ms_per_call": 1e3 * dt, "evals_per_s": P / dt, "frac_fp64_peak": f_alg / dt / 1e12 / FP64_PEAK_TFLOPS,
                         "plan_count_blocks_route": ctx.last_plan(), "alloc_s": ctx.alloc_stats()[0], "arena_gb": ctx.alloc_stats()[2] / 2 ** 30}
            ctx.close()
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    out["ragged_cohort_300_lognormal_D24"] = {"patients": P, "D": D, "Q": Q, "R": R, "n_median": int(np.median(ns)), "n_max": int(ns.max()),
                                              "sum_F_alg": f_alg, **res,
                                              "before_recorded": {"ms_per_call": 572.5, "source": "rounds 1-4 routing (MEDGP_NO_CLASSES=1), BENCH_r05.json / round-6 box; "
                                                                  "re-run with MEDGP_BENCH_RAGGED_BEFORE=1 (maps 166 GB)"},
                                              "speedup_vs_before": (res["before"]["ms_per_call"] if "before" in res else 572.5) / res["after"]["ms_per_call"]}


def config3_in_batch(out, dev_index, seed, reps):
    """What BASELINE config 3's lone N = 2048 patient costs where the reference's workload actually puts it (verdict r5 item 8): inside a
    lock-step batch of a cohort -- 255 patients of N = 263 (the heavy-tailed cohort's median) + the one of N = 2048, one nlml + gradient
    call, size classes on separate streams.  marginal = (call with it) - (call without it); standalone it is latency bound (0.86 ms,
    0.14 of peak: the diagonal chain of 32 look-ahead steps), in the batch the bulk's workgroups fill the CUs its chain leaves idle.
    ref for the workload: the job generator buckets patients by size, scripts/slurm_della.json:6-62."""
    import medgp_amd
    from medgp_amd import synth
    D, Q, R, NS, NL, PS = 24, 5, 8, 263, 2048, 255
    pts = [synth.patient(seed + 7, p, D, NS) for p in range(PS)] + [synth.patient(seed + 7, PS, D, NL)]
    th = np.stack([synth.theta(seed + 7, p, 7, Q, D, R) for p in range(PS + 1)])
    ctx = medgp_amd.Context(7, Q, D, R, device=dev_index)
    ctx.reserve(PS + 1, NL, PS + 1)
    ctx.set_patients(np.arange(PS + 1), pts)
    ctx.set_prior(-1, *synth.hier_gamma_prior(Q, D, R, 0.01))
    ctx.reserve_plan([NS] * PS + [NL])
    res = {}
    for name, sl in (("bulk_255xN263", np.arange(PS)), ("bulk_plus_1xN2048", np.arange(PS + 1)), ("alone_1xN2048", np.array([PS]))):
        nl, g, st = ctx.nlml_grad(sl, th[sl], True)
        assert np.all(st >= 0) and np.all(np.isfinite(nl)), name
        ctx.nlml_grad(sl, th[sl], True)
        t0 = time.perf_counter()
        for _ in range(4 * reps):
            ctx.nlml_grad(sl, th[sl], True)
        res[name] = {"ms_per_call": 1e3 * (time.perf_counter() - t0) / (4 * reps), "plan_count_blocks_route": ctx.last_plan()}
    ctx.close()
    out["config3_patient_inside_a_lockstep_batch"] = {**res, "marginal_ms_of_the_N2048_patient": res["bulk_plus_1xN2048"]["ms_per_call"] - res["bulk_255xN263"]["ms_per_call"],
                                                      "standalone_ms": res["alone_1xN2048"]["ms_per_call"]}


def screening(out, dev_index, seed, reps):
    import medgp_amd
    from medgp_amd import synth
    # random-init screening batch (ref: main_one_train.cpp:228-253): 1000 hyper vectors of ONE patient, nlml only
    D, N, Q, R, P = 24, 512, 5, 8, 1000
    ctx = medgp_amd.Context(7, Q, D, R, device=dev_index)
    ctx.reserve(1, N, P)
    ctx.set_patient(0, *synth.patient(seed + 2, 0, D, N))
    th = np.stack([synth.theta(seed + 2, s, 7, Q, D, R) for s in range(P)])
    slots = np.zeros(P, dtype=np.int32)
    nl, _, st = ctx.nlml_grad(slots, th, False)
    assert np.all(st >= 0) and np.all(np.isfinite(nl))
    ctx.nlml_grad(slots, th, False)
    t0 = time.perf_counter()
    for _ in range(reps):
        ctx.nlml_grad(slots, th, False)
    dt = (time.perf_counter() - t0) / reps
    ctx.profile_reset()
    ctx.profile_enable(True)
    ctx.nlml_grad(slots, th, False)
    prof = {k: round(v[0], 4) for k, v in ctx.profile_read().items() if v[1] > 0}
    out["screening_1000xN512_D24_nlml_only"] = {"evaluations": P, "N": N, "D": D, "ms_per_call": 1e3 * dt, "evals_per_s": P / dt,
                                                "frac_fp64_peak": (N ** 3 / 3 + 2 * N * N + 40 * Q * N * (N + 1) / 2) * P / dt / 1e12 / FP64_PEAK_TFLOPS,
                                                "kernel_ms": prof, "dominant_kernel": leg_roofline(prof, N, Q, D, synth.num_hyp(7, Q, D, R), P, nlml_only=True, shape="screening_1000xN512_nlml_only")}
    ctx.close()
    # the same evaluations through medgp_screen, the entry point the trainer uses (hyper block uploaded once, chunks queued without a
    # host wait, alternating between two lanes): 8 patients x 1000 vectors through max_batch 1024
    P8 = 8
    ctx = medgp_amd.Context(7, Q, D, R, device=dev_index)
    ctx.reserve(P8, N, 1024)
    ctx.set_patients(np.arange(P8), [synth.patient(seed + 2, p, D, N) for p in range(P8)])
    ctx.reserve_plan([N] * P8, P)
    nl8, st8 = ctx.screen(np.arange(P8), th)
    assert np.all(st8 >= 0) and np.array_equal(nl8[0], nl)            # patient 0: the bits of the call above
    t0 = time.perf_counter()
    for _ in range(reps):
        ctx.screen(np.arange(P8), th)
    dts = (time.perf_counter() - t0) / reps
    out["screening_1000xN512_D24_nlml_only"].update({"medgp_screen_8_patients_ms_per_1000": 1e3 * dts / P8, "medgp_screen_evals_per_s": P8 * P / dts,
                                                      "medgp_screen_frac_fp64_peak": (N ** 3 / 3 + 2 * N * N + 40 * Q * N * (N + 1) / 2) * P8 * P / dts / 1e12 / FP64_PEAK_TFLOPS})
    ctx.close()


def host_paths(out, dev_index, seed):
    """The callers either side of the hot path, end to end through the C++ hosts on the reference's file formats:
    cohort training (`medgp_train --pan-list`: random-init screening + lock-step SCG / varEM, ref: main_one_train.cpp) and the cohort
    online-imputation test (`medgp_test --pan-list`, both passes, ref: main_one_test.cpp:269-444).  Process wall clock of the
    executables on a synthetic experiment written here (the writing is not timed); reported beside the headline, never in it."""
    import re
    import shutil
    import subprocess
    import tempfile
    from medgp_amd import synth
    from medgp_amd.synth_experiment import make_experiment
    host = os.path.join(os.path.dirname(os.path.abspath(__file__)), "medgp_amd", "host")
    tmp = tempfile.mkdtemp(prefix="medgp_bench_host_")
    try:
        # ---- f1: 512 patients x N = 512, D = 24, Q = 5, R = 8, prior mode 2; 20 random initialisations, one varEM iteration of 8 SCG steps
        P, N, D, Q, R = 512, 512, 24, 5, 8
        pans = [f"P{k:04d}" for k in range(P)]
        ex = make_experiment(os.path.join(tmp, "train"), pans, D=D, Q=Q, R=R, N=N, feature_index=tuple(range(D)), seed=seed + 3,
                             opt=dict(random_init_num=20, top_iteration_num=1))
        plist = os.path.join(tmp, "train_pans.txt")
        open(plist, "w").write("\n".join(pans) + "\n")
        t0 = time.perf_counter()
        r = subprocess.run([os.path.join(host, "medgp_train"), "--cfg", ex["cfg"], "--pan-list", plist, "--thread", "1", "--device", str(dev_index)],
                           capture_output=True, text=True, timeout=600)
        wall = time.perf_counter() - t0
        if r.returncode != 0:
            raise RuntimeError("medgp_train rc %d: %s" % (r.returncode, (r.stdout + r.stderr)[-300:]))
        m1 = re.search(r"optimization finished: (\d+) nlml\+grad evaluations in (\d+) lock-step batches", r.stdout)
        m2 = re.search(r"lock-step optimisation: ([0-9.e+-]+) s wall \(([0-9.e+-]+) s waiting for the device", r.stdout)
        nout = len([f for f in os.listdir(ex["dirs"]["train"]) if f.startswith("train_")])
        out["train_cohort_512xN512_D24"] = {
            "patients": P, "N": N, "D": D, "random_init_num": 20, "process_wall_s": wall,
            "gradient_evaluations": int(m1.group(1)) if m1 else None, "lockstep_batches": int(m1.group(2)) if m1 else None,
            "lockstep_loop_s": float(m2.group(1)) if m2 else None, "device_wait_s": float(m2.group(2)) if m2 else None,
            "screening_evaluations": 20 * P, "output_files": nout}
        # ---- f1 at the reference's REAL budget (scripts/opt_prior2.json:3-6: 1000 random initialisations, 40 variational-EM iterations of
        #      30 SCG evaluations, early stop at < 0.5 % relative loss change, ref: util/c_optimizer_varEM.cpp:89-95): 2048 patients through
        #      1024 resident slots of ONE long-lived trainer (continuous admission, round 5)
        P2 = 2048
        pans2 = [f"B{k:05d}" for k in range(P2)]
        ex2 = make_experiment(os.path.join(tmp, "budget"), pans2, D=D, Q=Q, R=R, N=N, feature_index=tuple(range(D)), seed=seed + 5,
                              opt=dict(random_init_num=1000, top_iteration_num=40, iteration_num_per_update=30))
        plist2 = os.path.join(tmp, "budget_pans.txt")
        open(plist2, "w").write("\n".join(pans2) + "\n")
        t0 = time.perf_counter()
        r = subprocess.run([os.path.join(host, "medgp_train"), "--cfg", ex2["cfg"], "--pan-list", plist2, "--device", str(dev_index)],
                           capture_output=True, text=True, timeout=900)
        wall = time.perf_counter() - t0
        if r.returncode != 0:
            raise RuntimeError("medgp_train (real budget) rc %d: %s" % (r.returncode, (r.stdout + r.stderr)[-300:]))
        m1 = re.search(r"optimization finished: (\d+) nlml\+grad evaluations in (\d+) lock-step batches", r.stdout)
        m2 = re.search(r"lock-step optimisation: ([0-9.e+-]+) s wall \(([0-9.e+-]+) s waiting for the device", r.stdout)
        m3 = re.search(r"continuous admission: (\d+) patients through (\d+) resident slots in (\d+) admissions \(([0-9.e+-]+) s, of which screening ([0-9.e+-]+) s for (\d+) nlml-only", r.stdout)
        m4 = re.search(r"outside admissions: ([0-9.e+-]+); of the whole loop: ([0-9.e+-]+)", r.stdout)
        m5 = re.search(r"device memory: ([0-9.e+-]+) s in (\d+) management calls", r.stdout)
        out["train_cohort_2048xN512_D24_real_budget"] = {
            "alloc_s": float(m5.group(1)) if m5 else None,
            "patients": P2, "N": N, "D": D, "random_init_num": 1000, "top_iteration_num": 40, "iteration_num_per_update": 30,
            "process_wall_s": wall, "gradient_evaluations": int(m1.group(1)) if m1 else None, "lockstep_batches": int(m1.group(2)) if m1 else None,
            "loop_s": float(m2.group(1)) if m2 else None, "device_wait_s": float(m2.group(2)) if m2 else None,
            "resident_slots": int(m3.group(2)) if m3 else None, "admissions": int(m3.group(3)) if m3 else None,
            "admission_s": float(m3.group(4)) if m3 else None, "screening_s": float(m3.group(5)) if m3 else None,
            "screening_evaluations": int(m3.group(6)) if m3 else None,
            "screening_evals_per_s": (int(m3.group(6)) / float(m3.group(5))) if m3 and float(m3.group(5)) > 0 else None,
            "gradient_evals_per_s_outside_admissions": float(m4.group(1)) if m4 else None,
            "gradient_evals_per_s_whole_loop": float(m4.group(2)) if m4 else None,
            "output_files": len([f for f in os.listdir(ex2["dirs"]["train"]) if f.startswith("train_")])}
        # ---- the same trainer on a HEAVY-TAILED cohort at the real budget: 512 patients, log-normal sizes (median 263, max 5832): every
        #      lock-step batch and every screening chunk is a ragged call scheduled by size classes (round 5)
        P3 = 512
        ns3 = [max(48, int(v)) for v in synth.ragged_sizes(0, P3)]
        pans3 = [f"R{k:05d}" for k in range(P3)]
        ex3 = make_experiment(os.path.join(tmp, "ragged"), pans3, D=D, Q=Q, R=R, N=ns3, feature_index=tuple(range(D)), seed=seed + 6,
                              opt=dict(random_init_num=1000, top_iteration_num=40, iteration_num_per_update=30))
        plist3 = os.path.join(tmp, "ragged_pans.txt")
        open(plist3, "w").write("\n".join(pans3) + "\n")
        def ragged_run():
            for f in os.listdir(ex3["dirs"]["train"]):
                if f.startswith("train_"):
                    os.remove(os.path.join(ex3["dirs"]["train"], f))
            t0 = time.perf_counter()
            r = subprocess.run([os.path.join(host, "medgp_train"), "--cfg", ex3["cfg"], "--pan-list", plist3, "--resident", "512", "--device", str(dev_index)],
                               capture_output=True, text=True, timeout=900)
            wall = time.perf_counter() - t0
            if r.returncode != 0:
                raise RuntimeError("medgp_train (ragged, real budget) rc %d: %s" % (r.returncode, (r.stdout + r.stderr)[-300:]))
            m1 = re.search(r"optimization finished: (\d+) nlml\+grad evaluations in (\d+) lock-step batches", r.stdout)
            m3 = re.search(r"continuous admission: (\d+) patients through (\d+) resident slots in (\d+) admissions \(([0-9.e+-]+) s, of which screening ([0-9.e+-]+) s for (\d+) nlml-only", r.stdout)
            m4 = re.search(r"outside admissions: ([0-9.e+-]+); of the whole loop: ([0-9.e+-]+)", r.stdout)
            m5 = re.search(r"device memory: ([0-9.e+-]+) s in (\d+) management calls \(([0-9.e+-]+) s of it announcing the sizes up front\), ([0-9.e+-]+) GB held", r.stdout)
            return {"process_wall_s": wall, "gradient_evaluations": int(m1.group(1)) if m1 else None,
                    "lockstep_batches": int(m1.group(2)) if m1 else None, "screening_s": float(m3.group(5)) if m3 else None,
                    "screening_evaluations": int(m3.group(6)) if m3 else None,
                    "gradient_evals_per_s_outside_admissions": float(m4.group(1)) if m4 else None,
                    "alloc_s": float(m5.group(1)) if m5 else None, "alloc_calls": int(m5.group(2)) if m5 else None,
                    "reserve_plan_s": float(m5.group(3)) if m5 else None, "arena_gb": float(m5.group(4)) if m5 else None,
                    "trained": sum(open(os.path.join(ex3["dirs"]["train"], f"train_flag_{p}.txt")).read().strip() == "1" for p in pans3)}
        first = ragged_run()
        second = ragged_run()     # the same run again: the two must agree (round 5's varied 2 x with what the device memory had been used for)
        out["train_cohort_512_lognormal_D24_real_budget"] = {
            "patients": P3, "n_median": int(np.median(ns3)), "n_max": int(max(ns3)), "D": D, "random_init_num": 1000, "top_iteration_num": 40,
            "iteration_num_per_update": 30, **first, "repeat": second,
            "repeat_wall_ratio": second["process_wall_s"] / first["process_wall_s"]}
        # ---- BASELINE config 1 as SURVEY 8d defines it: the REFERENCE-WRITTEN exp_setup.json / hyp_bound.txt / mode kernel (D = 2, Q = 5,
        #      R = 2, H = 42, 1000 + 5 x 100 + 35 x 30), one patient of 75 + 75 observations, medgp_train then medgp_test (both passes);
        #      parity of exactly this run: tests/test_config1_gpu.py
        from medgp_amd.synth_experiment import reference_config1_tree
        cwd1, cfg1, _, _, _ = reference_config1_tree(os.path.join(tmp, "config1"), os.path.dirname(os.path.abspath(__file__)))
        t0 = time.perf_counter()
        r = subprocess.run([os.path.join(host, "medgp_train"), "--cfg", cfg1, "--pan", "PT0001", "--thread", "1", "--device", str(dev_index)],
                           capture_output=True, text=True, timeout=600, cwd=cwd1)
        wall_tr = time.perf_counter() - t0
        if r.returncode != 0:
            raise RuntimeError("medgp_train (config 1) rc %d: %s" % (r.returncode, (r.stdout + r.stderr)[-300:]))
        m1 = re.search(r"optimization finished: (\d+) nlml\+grad evaluations in (\d+) lock-step batches", r.stdout)
        t0 = time.perf_counter()
        r = subprocess.run([os.path.join(host, "medgp_test"), "--cfg", cfg1, "--pan", "PT0001", "--thread", "1", "--fold", "0", "--kernclust-alg", "gmm",
                            "--device", str(dev_index)], capture_output=True, text=True, timeout=600, cwd=cwd1)
        wall_te = time.perf_counter() - t0
        if r.returncode != 0:
            raise RuntimeError("medgp_test (config 1) rc %d: %s" % (r.returncode, (r.stdout + r.stderr)[-300:]))
        out["config1_PT_INR_N150"] = {"patients": 1, "N": 150, "D": 2, "Q": 5, "R": 2, "H": 42, "random_init_num": 1000, "top_iteration_num": 40,
                                      "train_process_wall_s": wall_tr, "gradient_evaluations": int(m1.group(1)) if m1 else None,
                                      "test_process_wall_s": wall_te, "imputations_per_pass": [int(v) for v in re.findall(r"INFO: (\d+) imputations in", r.stdout)],
                                      "config": "tests/golden/ref_cfg/PT_INR/exp_setup.json as the reference's config.py wrote it"}
        # ---- f3: 64 test patients, D = 4, N 120 .. 200, both passes (with / without the online hyper updates)
        P, D, Q, R = 64, 4, 3, 2
        pans = [f"C{k:03d}" for k in range(P)]
        ns = [int(v) for v in np.random.default_rng(seed + 4).integers(120, 201, size=P)]
        ex = make_experiment(os.path.join(tmp, "test"), pans, D=D, Q=Q, R=R, N=ns, feature_index=(18, 19, 20, 21), seed=seed + 4,
                             opt={"online_learn_rate": 1e-4})
        fold = os.path.join(ex["dirs"]["kernel"], "fold0")
        os.makedirs(fold)
        open(os.path.join(fold, "gmm_mode_mixture_num.txt"), "w").write(f"{Q}\n")
        synth.theta(9, 0, 7, Q, D, R).tofile(os.path.join(fold, "gmm_mode_param.bin"))
        plist = os.path.join(tmp, "test_pans.txt")
        open(plist, "w").write("\n".join(pans) + "\n")
        t0 = time.perf_counter()
        r = subprocess.run([os.path.join(host, "medgp_test"), "--cfg", ex["cfg"], "--pan-list", plist, "--thread", "1", "--fold", "0",
                            "--kernclust-alg", "gmm", "--device", str(dev_index)], capture_output=True, text=True, timeout=600)
        wall = time.perf_counter() - t0
        if r.returncode != 0:
            raise RuntimeError("medgp_test rc %d: %s" % (r.returncode, (r.stdout + r.stderr)[-300:]))
        m1 = re.search(r"hyper trajectories: (\d+) gradient evaluations in (\d+) batched calls \((\d+) lock-step rounds\) ([0-9.e+-]+) ms", r.stdout)
        imps = [int(v) for v in re.findall(r"INFO: (\d+) imputations in", r.stdout)]
        m3 = re.search(r"pass wall time: without updating ([0-9.e+-]+) ms, with updating ([0-9.e+-]+) ms", r.stdout)
        out["test_cohort_64xN120-200_D4"] = {
            "patients": P, "D": D, "process_wall_s": wall,
            "update_pass_gradient_evaluations": int(m1.group(1)) if m1 else None, "update_pass_rounds": int(m1.group(3)) if m1 else None,
            "trajectory_ms": float(m1.group(4)) if m1 else None, "imputations_per_pass": imps,
            "pass_ms_without_update": float(m3.group(1)) if m3 else None, "pass_ms_with_update": float(m3.group(2)) if m3 else None}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def config4_full(out, dev_index, seed, reps=3):
    """BASELINE config 4 as it is NAMED -- the fixed cohort of 4096 patients x N=512, D=24 -- on ONE GPU (what `--scaling strong`
    gives rank 0 at N=1; at N=8 it coincides with the headline's 512-patient shard).  Device-pointer API like the headline,
    hier-gamma prior, nlml + gradient; measured two ways: one call of 4096 evaluations, and 8 calls of 512 back to back."""
    import torch
    import medgp_amd
    from medgp_amd import synth
    D, N, Q, R, P = 24, 512, 5, 8, 4096
    H = synth.num_hyp(7, Q, D, R)
    dev = torch.device("cuda", dev_index)
    ctx = medgp_amd.Context(7, Q, D, R, device=dev_index)
    ctx.reserve(P, N, P)
    pts = [synth.patient(seed, s, D, N) for s in range(P)]
    thetas = np.stack([synth.theta(seed, s, 7, Q, D, R) for s in range(P)])
    ctx.set_patients(np.arange(P), pts)
    ctx.set_prior(-1, *synth.hier_gamma_prior(Q, D, R, 0.01))
    theta_d = torch.from_numpy(thetas).to(dev)
    nlml_d = torch.empty(P, dtype=torch.float64, device=dev)
    grad_d = torch.empty((P, H), dtype=torch.float64, device=dev)
    stat_d = torch.empty(P, dtype=torch.int32, device=dev)
    slots = np.arange(P, dtype=np.int32)

    def one_call():
        ctx.nlml_grad_device(slots, theta_d.data_ptr(), 1, nlml_d.data_ptr(), grad_d.data_ptr(), stat_d.data_ptr())

    def eight_calls():
        for c in range(8):
            a, b = 512 * c, 512 * (c + 1)
            ctx.nlml_grad_device(slots[a:b], theta_d[a:b].data_ptr(), 1, nlml_d[a:b].data_ptr(), grad_d[a:b].data_ptr(), stat_d[a:b].data_ptr())

    res = {}
    for name, fn in (("one_call_of_4096", one_call), ("eight_calls_of_512", eight_calls)):
        fn()
        ctx.synchronize()
        assert bool((stat_d >= 0).all()) and bool(torch.isfinite(nlml_d).all()), name
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        ctx.synchronize()
        dt = (time.perf_counter() - t0) / reps
        res[name] = {"ms_per_cohort_pass": 1e3 * dt, "evals_per_s": P / dt}
    best = min(res, key=lambda k: res[k]["ms_per_cohort_pass"])
    f_alg = N ** 3 + 6 * N * N + 80 * Q * N * (N + 1) / 2
    out["config4_full_4096xN512_D24"] = {"patients": P, "N": N, "D": D, "Q": Q, "R": R, "H": H, "n_gpus": 1, **res, "faster": best,
                                         "evals_per_s": res[best]["evals_per_s"],
                                         "frac_fp64_peak": f_alg * res[best]["evals_per_s"] / 1e12 / FP64_PEAK_TFLOPS}
    ctx.close()


def cohort_kde(out, dev_index, seed):
    # cohort mode estimation: the KDE modes of one cluster of a 4096-subject cohort at D = 24
    # (24 nuggets + mu + v + 300 elements of B; one exp per sample pair -- VALU bound)
    from medgp_amd import capi
    rng = np.random.default_rng(seed)
    Pc, ns = 4096, 24 + 2 + 300
    series = [rng.normal(size=Pc) * rng.uniform(0.1, 3.0) for _ in range(ns)]
    capi.kde_mode(series[:8], True, dev_index)
    t0 = time.perf_counter()
    _, _, st, kms = capi.kde_mode(series, True, dev_index, full=True)
    dt = time.perf_counter() - t0
    assert np.all(st == 0)
    out["cohort_mode_kde_P4096_D24_one_cluster"] = {"series": ns, "samples_per_series": Pc, "kernel_ms": kms, "call_ms": 1e3 * dt,
                                                     "gaussian_pair_terms_per_s": ns * Pc * Pc / (kms * 1e-3)}


def resolve_launch(gpus, env, argv, run=None):
    """None: go on in this process.  Otherwise the exit code to leave with: 2 after a mismatch between --gpus and the launcher's
    WORLD_SIZE (message on stderr, no JSON line), or the exit code of the N-rank launch this process started and waited for."""
    under_launcher = all(k in env for k in ("RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"))
    if under_launcher:
        if int(env["WORLD_SIZE"]) != gpus:
            if env.get("RANK", "0") == "0":
                print(f"bench.py: --gpus {gpus} but the launcher started WORLD_SIZE={env['WORLD_SIZE']} ranks; refusing to print a line whose n_gpus "
                      f"differs from --gpus", file=sys.stderr, flush=True)
            return 2
        return None
    if gpus <= 1:
        return None
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    print(f"bench.py: --gpus {gpus} without a launcher: starting {gpus} ranks: {' '.join(cmd)}", file=sys.stderr, flush=True)
    return (run or subprocess.call)(cmd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--patients", type=int, default=512, help="patients per GPU")
    ap.add_argument("--n", "--obs", dest="n", type=int, default=512, help="observations per patient (--obs: spelling that survives torch.distributed.run's prefix matching)")
    ap.add_argument("--D", type=int, default=24)
    ap.add_argument("--Q", type=int, default=5)
    ap.add_argument("--R", type=int, default=8)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-prior", action="store_true")
    ap.add_argument("--flag-grad", type=int, default=1)
    ap.add_argument("--no-extra", action="store_true", help="skip the short measurements of BASELINE configs 2, 3, 5")
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak",
                    help="weak: --patients per GPU (default); strong: the fixed --cohort (BASELINE config 4: 4096 patients) LPT-sharded over the ranks")
    ap.add_argument("--cohort", type=int, default=4096, help="cohort size of --scaling strong")
    ap.add_argument("--backend", choices=("auto", "nccl", "gloo"), default="auto",
                    help="process-group backend for N > 1: auto = nccl (RCCL) with one rank per GPU, gloo when ranks share GPUs")
    ap.add_argument("--dump-results", default=None, help="write this rank's (global patient ids, nlml, gradient row sums) to <path>.rank<r>.npz")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the last timed step computed (nlml, gradient, status per patient, with the patients' global ids) as "
                         "DIR/<name>.npy in float64; more than 64 MB: a fixed, seeded sample of the patients")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: roofline and per-kernel split of the step, sustained rate, "
                         "BASELINE configs 2, 3, 5 and the other legs (--no-extra skips them), CPU baseline (--no-cpu-baseline skips it)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    # --gpus N is the contract: a line whose n_gpus differs from it must never be printed (verdict r5 item 7).  Under a launcher
    # (torch.distributed.run's environment) N must equal WORLD_SIZE.  Without one and N > 1 this process starts the N ranks ITSELF --
    # as children of a parent that has not touched the GPU (no torch import above this line) and only waits and passes their output
    # through; the reference's fan-out being replaced is one scheduler job per patient (medgpc/util/run_exp_generator.py:213-260).
    rc = resolve_launch(args.gpus, os.environ, sys.argv[1:])
    if rc is not None:
        sys.exit(rc)

    import torch
    import medgp_amd
    from medgp_amd import synth

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    ndev = torch.cuda.device_count()
    # launched by torch.distributed.run (its environment is there): the process group is created even for ONE rank, so that a
    # `--nproc-per-node 1` launch on a one-GPU box runs the very code path of the 8-GPU run -- RCCL initialisation, barrier, all-reduce,
    # all-gather -- instead of leaving it untested (plain `python bench.py` has no such environment and no group)
    use_dist = world > 1 or all(k in os.environ for k in ("RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"))
    if use_dist:
        import torch.distributed as dist
        backend = args.backend if args.backend != "auto" else ("nccl" if ndev >= world else "gloo")
        if backend == "nccl":   # the driver's case: one rank per GPU, RCCL over xGMI
            if ndev < world:
                sys.exit(f"bench.py: --backend nccl needs one GPU per rank ({world} ranks, {ndev} GPUs visible)")
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:                   # gloo: also with more ranks than GPUs (testing the multi-rank path on a 1-GPU box): ranks share devices
            local_rank = local_rank % max(ndev, 1)
            torch.cuda.set_device(local_rank)
            dist.init_process_group("gloo")
    else:
        torch.cuda.set_device(0)
        local_rank = 0
    dev = torch.device("cuda", local_rank)

    D, N, Q, R, P = args.D, args.n, args.Q, args.R, args.patients
    H = synth.num_hyp(7, Q, D, R)
    if args.scaling == "strong":
        # fixed cohort, static LPT partition by the per-patient cost N^3 + 80 Q N^2 / 2 (uniform N: contiguous-size shards);
        # ref: one scheduler job per patient, medgpc/util/run_exp_generator.py:213-260
        from medgp_amd import shard
        gids = shard.lpt_partition([N] * args.cohort, world, Q)[rank]
        P = int(gids.size)
    else:
        gids = np.arange(rank * P, (rank + 1) * P, dtype=np.int64)   # weak scaling: rank r owns global patients [r*P, (r+1)*P)
    ctx = medgp_amd.Context(7, Q, D, R, device=local_rank)
    ctx.reserve(P, N, P)
    thetas = np.empty((P, H))
    pts = []
    for s in range(P):
        pts.append(synth.patient(args.seed, int(gids[s]), D, N))
        thetas[s] = synth.theta(args.seed, int(gids[s]), 7, Q, D, R)
    ctx.set_patients(np.arange(P), pts)     # packed upload: one transfer for the whole shard
    if not args.no_prior:
        ctx.set_prior(-1, *synth.hier_gamma_prior(Q, D, R, 0.01))
    slots = np.arange(P, dtype=np.int32)
    theta_d = torch.from_numpy(thetas).to(dev)
    nlml_d = torch.empty(P, dtype=torch.float64, device=dev)
    grad_d = torch.empty((P, H), dtype=torch.float64, device=dev)
    stat_d = torch.empty(P, dtype=torch.int32, device=dev)

    def step():
        ctx.nlml_grad_device(slots, theta_d.data_ptr(), args.flag_grad, nlml_d.data_ptr(), grad_d.data_ptr(), stat_d.data_ptr())

    def barrier():
        if use_dist:
            import torch.distributed as dist
            dist.barrier()

    if args.full:
        # the warm-up steps run with events around every launch: they say which kernel dominates the step
        ctx.profile_reset()
        ctx.profile_enable(True)
        for _ in range(args.warmup):
            step()
        ctx.synchronize()
        torch.cuda.synchronize()
        prof_w = ctx.profile_read() if args.warmup > 0 else {}
        ctx.profile_enable(False)
        if not prof_w:
            # --warmup 0: the dominant kernel is still MEASURED, by one untimed profiled step -- a default name would bracket the wrong
            # kernel on look-ahead shapes (few large patients), where k_cholinv is only the retry launch that does nothing
            ctx.profile_reset()
            ctx.profile_enable(True)
            step()
            ctx.synchronize()
            prof_w = ctx.profile_read()
            ctx.profile_enable(False)
        tot_w = {k: v[0] for k, v in prof_w.items() if v[1] > 0}
        dom_kernel = max(tot_w, key=tot_w.get)
        # HIP events on the launch stream, live over the timed region, around the launches of the DOMINANT kernel only (the
        # roofline leg): events around all seven launches of a step cost 1.6 % of it (scratch/prof_overhead.py).  The other kernels'
        # per-step times are taken in a short pass behind the timed region (kernel_ms_per_step), with events around every launch.
        ctx.profile_reset()
        ctx.profile_enable(True, only=dom_kernel)
    else:
        # a plain run: no events anywhere, the headline needs none
        for _ in range(args.warmup):
            step()
        ctx.synchronize()
        torch.cuda.synchronize()
    barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    ctx.synchronize()
    torch.cuda.synchronize()
    barrier()
    t_local = time.perf_counter() - t0
    if args.full:
        prof = ctx.profile_read()
        ctx.profile_enable(False)
    t = aggregate_time(t_local, world)

    # the last timed step's results, read before anything else runs on these buffers
    st = stat_d.cpu().numpy()
    nl = nlml_d.cpu().numpy()
    grad = grad_d.cpu().numpy() if (args.dump_outputs or args.dump_results) else None
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, gids, {"nlml": nl, "grad": grad, "status": st},
                     suffix="" if world == 1 else f"_rank{rank}", limit=DUMP_LIMIT_BYTES // world)
    assert np.all(st >= 0) and np.all(np.isfinite(nl)), "evaluation failed inside the timed region"
    if args.full:
        # per-kernel split of a step (untimed): a few more steps with events around every launch
        ctx.profile_reset()
        ctx.profile_enable(True)
        n_split = max(3, min(args.steps, 10))
        for _ in range(n_split):
            step()
        ctx.synchronize()
        prof_all = ctx.profile_read()
        ctx.profile_enable(False)

    if args.dump_results:
        np.savez(f"{args.dump_results}.rank{rank}.npz", gids=gids, nlml=nl, gsum=grad.sum(axis=1), status=st)
    # who actually ran: (rank, device index, device name, uuid, host) of every rank, gathered once outside the timed region
    props = torch.cuda.get_device_properties(local_rank)
    me = {"rank": rank, "device": local_rank, "name": props.name, "uuid": str(getattr(props, "uuid", "")),
          "host": os.uname().nodename, "patients": int(P), "ms_per_step": 1e3 * t_local / max(args.steps, 1)}
    if use_dist:
        import torch.distributed as dist
        seen = [None] * world
        dist.all_gather_object(seen, me)
        backend = dist.get_backend()
    else:
        seen, backend = [me], "none"
    # One rank per GPU is what the scaling numbers mean: under nccl every rank must sit on a device of its own.  Two ranks on one
    # device would still produce a line (half the per-rank rate each) -- refuse instead of reporting it.
    problem = check_ranks(seen, world, backend)
    if problem:
        if rank == 0:
            print("bench.py: " + problem, file=sys.stderr, flush=True)
        ctx.close()
        if use_dist:
            dist.destroy_process_group()
        sys.exit(3)

    if rank == 0:
        total_patients = sum(r["patients"] for r in seen)
        value = total_patients * args.steps / t
        f_alg = N ** 3 + 6 * N * N + 80 * Q * N * (N + 1) / 2
        rank_ms = [r["ms_per_step"] for r in seen]
        try:   # RCCL's version when the nccl backend carried the barrier / reductions (verdict r5 item 5)
            nccl_version = ".".join(str(v) for v in torch.cuda.nccl.version()) if backend == "nccl" else None
        except Exception:   # noqa: BLE001
            nccl_version = None
        extra = {
            "ranks_seen": seen, "backend": backend, "nccl_version": nccl_version,
            "rank_ms_per_step": {"min": min(rank_ms), "max": max(rank_ms), "mean": sum(rank_ms) / len(rank_ms)},
            "end_to_end": {"flop_per_eval": f_alg, "tflops": f_alg * value / world / 1e12,
                           "frac_fp64_peak": f_alg * value / world / 1e12 / FP64_PEAK_TFLOPS},
        }
        if args.full:
            extra["roofline"] = step_roofline(prof, prof_all, n_split, N, Q, D, H, P)
        if args.full and world == 1 and not args.no_extra and (P, N, D) == (512, 512, 24):
            # sustained rate: the timed region above is tens of milliseconds; this repeats the same step back to back for >= 2 s
            # (clocks settle under load) -- reported beside the headline, never instead of it
            try:
                n_s, t_s0 = 0, time.perf_counter()
                while True:
                    for _ in range(50):
                        step()
                    ctx.synchronize()
                    n_s += 50
                    if time.perf_counter() - t_s0 >= 2.0:
                        break
                dt_s = time.perf_counter() - t_s0
                extra["sustained"] = {"seconds": dt_s, "steps": n_s, "ms_per_step": 1e3 * dt_s / n_s, "evals_per_s": P * n_s / dt_s}
            except Exception as e:   # noqa: BLE001
                extra["sustained"] = {"error": str(e)[:200]}
            extra["other_configs"] = other_configs(local_rank, args.seed)
        if args.full and world == 1 and not args.no_cpu_baseline:
            extra["cpu_baseline"] = cpu_baseline(D, N, Q, R, args.seed)
        what = (f"config 4 cohort: {total_patients} patients LPT-sharded over {world} GPU(s) ({P} on rank 0)" if args.scaling == "strong"
                else f"config 4 shard: {P} patients/GPU")
        line = result_line(value, world, args.steps, args.warmup, 1e3 * t / args.steps,
                           f"{what} x N={N}, D={D}, Q={Q}, R={R}, H={H}, LMC-SM + hier-gamma prior, nlml+grad",
                           extra, scaling=args.scaling)
        line["config"].update({"patients_per_gpu": P, "cohort": total_patients, "N": N, "D": D, "Q": Q, "R": R, "H": H,
                               "parallelism": f"patient-sharded x{world} (no collective)"})
        print(json.dumps(line), flush=True)
    ctx.close()
    if use_dist:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
