"""FCX_OPT_ATMOS_INVARIANT through the product's own exchange (fcx_atmos_allreduce, atmos_exchange)
with 2 and 3 processes on the one GPU, the mock RCCL standing in for librccl.so exactly as in
tests/test_gpu_exchange_ranks.py (a host-memory all-reduce that fails instead of waiting).

N = 24,012: every APPLE cut of 2 and 3 ranks falls inside an atmosphere cell.  Every atmosphere
cell on every rank must have the BITS of a one-rank engine that rank 0 runs over the global grid;
the ranks' collective call logs are identical, ONE fp64 sum all-reduce per exchange whose count
is sum(n_boundaries x fields x (1 + K)); a default run (the option off) has the parent's counts;
ranks that disagree on K all get the named signature error and none hangs.  Each process runs
under its own time limit and the parent checks every exit status."""
import dataclasses
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, "components.flux_calculator_amd", "lib", "test", "libmock_rccl.so")
FIELDS = (("MEVA", 1), ("HLAT", 1), ("HSEN", 1), ("RBBR", 1), ("UMOM", 2), ("VMOM", 3))
VARIANTS = ("CCLM", "MOM5", "RCO")
N = 24_012

# (name, slot layout, streams, special)
SCENARIOS = [
    ("adjacent_one_stream", "adjacent", "one", None),
    ("separate_engine_streams", "separate", "per_engine", None),
    ("group_one_exchange", "own", "one", "group"),
    # fcx_set_comm: every engine completes its own slots inside fcx_run (engine 1 not fused and
    # with FCX_OPT_ATMOS_IN_RUN 0: inside fcx_run_atmos), and inside fcx_run_group
    ("attached_comm", "own", "one", "attached"),
    ("attached_group", "own", "one", "attached_group"),
    ("default_option_off", "adjacent", "one", "off"),
    ("max_terms_mismatch", "adjacent", "one", "mismatch"),
]
SCENARIOS_3 = [
    ("rank_inside_one_cell", "adjacent", "one", "tiny_middle"),
    ("empty_middle_rank", "separate", "one", "empty_middle"),
]


def _uid():
    name = f"/fcxmock-inv-{os.getpid()}-{np.random.default_rng().integers(1 << 62):x}".encode()
    return name + b"\0" * (128 - len(name))


def _ranges(world, special, amap):
    from fcx.parallel import apple_range

    idx, n = amap.atmos_index, amap.atmos_index.shape[0]
    if special == "empty_middle":
        k = next(i for i in range(n // 2, n) if idx[i - 1] == idx[i])
        return [(0, k), (0, 0), (k, n - k)]
    if special == "tiny_middle":
        starts = np.flatnonzero(np.diff(np.concatenate([[-1], idx])))  # first cell of each run
        lens = np.diff(np.concatenate([starts, [n]]))
        c0 = int(starts[np.flatnonzero(lens >= 4)[len(starts) // 3 // 2]])
        return [(0, c0 + 1), (c0 + 1, 2), (c0 + 3, n - c0 - 3)]
    return [apple_range(n, r, world) for r in range(world)]


def _scenario(rank, world, uid, name, layout, streams, special, log):
    import torch
    from fcx.basic import PHASE_ALL, PHASE_NORMAL
    from fcx.comm import Comm
    from fcx.engine import Engine, run_group
    from fcx.parallel import local_atmos, synthetic_atmos_map
    from fcx.synthetic import build_case
    from test_gpu_multirank import shard_case

    os.environ["FCX_MOCK_RCCL_LOG"] = log
    amap = synthetic_atmos_map(N)
    ranges = _ranges(world, special, amap)
    la = local_atmos(amap, rank, world, ranges=ranges)
    invariant = special != "off"
    if special == "mismatch" and rank == 1:
        la = dataclasses.replace(la, max_terms=la.max_terms + 1)  # this rank's K differs
    off, size = ranges[rank]
    nb = world - 1
    stride = len(FIELDS) * (1 + la.max_terms) if invariant else len(FIELDS)
    region = nb * stride
    dev = "cuda:0"
    if layout == "adjacent":
        big = torch.zeros(3 * region, dtype=torch.float64, device=dev)
        slots, bufs = [big[i * region:] for i in range(3)], [big]
    elif layout == "separate":
        bufs = slots = [torch.zeros(region, dtype=torch.float64, device=dev) for _ in range(3)]
    else:
        bufs, slots = [], [None] * 3
    own = [torch.cuda.Stream() for _ in range(3)] if streams == "per_engine" else [torch.cuda.current_stream()] * 3
    comm = Comm(0, world, rank, uid)
    engines, cases, outs_all = [], [], []
    # rank 0 also runs the oracle: ONE engine per variant over the global grid, the option off
    oracle = []
    for i, v in enumerate(VARIANTS):
        full = build_case(v, n=N, T=1, bias=True, seed=41 + i)
        case = shard_case(full, off, off + size, v, seed=41 + i)
        outs = {f: torch.full((max(la.n_atmos, 1),), float("nan"), dtype=torch.float64, device=dev) for f, _ in FIELDS}
        atmos = {"local": la, "fields": [(PHASE_NORMAL, 1, g, f, outs[f]) for f, g in FIELDS], "invariant": invariant}
        if layout == "own":
            atmos["own_boundaries"] = True
        else:
            atmos["shared"] = (slots[i], stride)
        opts = None
        if special in ("attached", "attached_group"):
            atmos["comm"] = comm
        if special == "attached" and i == 1:
            opts = {"atmos_in_run": 0, "specialize": 0}  # the accumulation, terms and exchange in fcx_run_atmos
        e = Engine(case.lf, 1, case.methods, corrections=case.corrections, atmos=atmos, stream=own[i].cuda_stream,
                   options=opts)
        assert e.atmos_columns() == stride
        e.upload(PHASE_ALL)
        engines.append(e)
        cases.append(case)
        outs_all.append(outs)
        if rank == 0 and special != "mismatch":
            g_outs = {f: torch.full((amap.n_atmos,), float("nan"), dtype=torch.float64, device=dev) for f, _ in FIELDS}
            g = Engine(full.lf, 1, full.methods, corrections=full.corrections,
                       atmos={"local": local_atmos(amap, 0, 1),
                              "fields": [(PHASE_NORMAL, 1, gg, f, g_outs[f]) for f, gg in FIELDS]})
            g.upload(PHASE_ALL)
            oracle.append((g, g_outs))
    torch.cuda.synchronize()
    result = {"name": name, "atmos_offset": la.atmos_offset, "n_atmos": la.n_atmos, "left": la.left,
              "right": la.right, "left_pos": la.left_pos, "max_terms": la.max_terms, "stride": stride, "nb": nb,
              "steps": []}
    for step in range(2):
        for outs in outs_all:
            for o in outs.values():
                o.fill_(float("nan"))
        torch.cuda.synchronize()
        err, group = None, None
        if special in ("group", "attached_group"):
            run_group(engines, PHASE_ALL, 3600 * step)
            group = [e.last_group_size() for e in engines]
        else:
            for i, e in enumerate(engines):
                e.run(PHASE_ALL, 3600 * step)
                if special == "attached" and i == 1:
                    assert e.last_terms_group() == 0  # nothing accumulated yet
                    e.run_atmos(PHASE_ALL)
        terms = [e.last_terms_group() for e in engines]
        try:
            if special not in ("attached", "attached_group"):
                comm.atmos_allreduce(engines)
        except Exception as ex:  # noqa: BLE001 -- reported to the parent
            err = str(ex)
        for e in engines:
            e.synchronize()
        torch.cuda.synchronize()
        rec = {"error": err, "group": group, "terms": terms, "slots_zero": all(float(b.abs().sum()) == 0.0 for b in bufs),
               "out": [{f: outs[f].cpu().numpy()[: la.n_atmos].copy() for f, _ in FIELDS} for outs in outs_all],
               "oracle": []}
        for g, g_outs in oracle:
            g.run(PHASE_ALL, 3600 * step)
            g.synchronize()
            rec["oracle"].append({f: g_outs[f].cpu().numpy().copy() for f, _ in FIELDS})
        result["steps"].append(rec)
        if special == "mismatch":
            break
    for e in engines + [g for g, _ in oracle]:
        e.close()
    comm.close()
    return result


def _child(rank, world, uids, scenarios, logdir, q):
    os.environ["FCX_RCCL_LIBRARY"] = MOCK
    os.environ["FCX_MOCK_RCCL_TIMEOUT_S"] = "30"
    try:
        import torch

        torch.cuda.set_device(0)
        out = []
        for (name, layout, streams, special), uid in zip(scenarios, uids):
            out.append(_scenario(rank, world, uid, name, layout, streams, special, os.path.join(logdir, name)))
        q.put((rank, None, out))
    except Exception as ex:  # noqa: BLE001
        import traceback

        q.put((rank, traceback.format_exc() + repr(ex), None))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("world", [2, 3])
def test_invariant_ranks_through_libfcx(world, tmp_path):
    import torch.multiprocessing as mp

    assert os.path.exists(MOCK), "build() makes the mock RCCL (make -C components.flux_calculator_amd mock-rccl)"
    scenarios = SCENARIOS + (SCENARIOS_3 if world == 3 else [])
    uids = [_uid() for _ in scenarios]
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    procs = [ctx.Process(target=_child, args=(r, world, uids, scenarios, str(tmp_path), q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(world):
        rank, err, out = q.get()
        assert err is None, f"rank {rank}: {err}"
        res[rank] = out
    for p in procs:
        p.join(timeout=120)  # each process under its own time limit, every exit status checked
        assert p.exitcode == 0
    problems = []
    for k, (name, layout, streams, special) in enumerate(scenarios):
        per = [res[r][k] for r in range(world)]
        logs = [open(os.path.join(tmp_path, name) + f".{r}").read() for r in range(world)]
        if special == "mismatch":
            errs = [p["steps"][0]["error"] for p in per]
            if not all(e and "ranks disagree" in e for e in errs):
                problems.append(f"{name}: expected every rank to report the disagreement, got {errs}")
            continue
        if len(set(logs)) != 1:
            problems.append(f"{name}: call sequences differ: {logs}")
        # the collective: one agreement (6 doubles, max) before the first exchange, then ONE sum
        # all-reduce per step of sum(n_boundaries x stride) doubles
        sums = [ln.split() for ln in logs[0].splitlines() if ln.endswith(" sum")]
        attached = special in ("attached", "attached_group")
        count = per[0]["nb"] * per[0]["stride"] * (1 if attached else 3)
        want_sums = [count] * (6 if attached else 2)  # attached: every engine's own exchange, each step
        want_stride = len(FIELDS) if special == "off" else len(FIELDS) * (1 + per[0]["max_terms"])
        if per[0]["stride"] != want_stride or [int(s[1]) for s in sums] != want_sums:
            problems.append(f"{name}: sum all-reduces {sums}, want {want_sums} doubles (stride {want_stride})")
        # the terms launches: ONE for the engines of an fcx_run_group, one each where an engine
        # runs or exchanges by itself, none with the option off (a rank without a shared cell: 0)
        for r, p in enumerate(per):
            has = p["left"] >= 0 or p["right"] >= 0
            want_t = [0 if (special == "off" or not has) else 3 if special == "group" else 1] * 3
            if any(st["terms"] != want_t for st in p["steps"]):
                problems.append(f"{name} rank {r}: terms launch sizes {[st['terms'] for st in p['steps']]}, want {want_t}")
        if sum(ln.endswith(" max") for ln in logs[0].splitlines()) != 1:
            problems.append(f"{name}: expected one signature agreement, log {logs[0]!r}")
        if special in ("group", "attached_group") and any(st["group"] != [3, 3, 3] for p in per for st in p["steps"]):
            problems.append(f"{name}: group sizes {[st['group'] for p in per for st in p['steps']]}")
        shared, differing = 0, 0
        for step in range(2):
            for p in per:
                if p["steps"][step]["error"]:
                    problems.append(f"{name} step {step}: {p['steps'][step]['error']}")
                if not p["steps"][step]["slots_zero"]:
                    problems.append(f"{name} step {step}: slots not re-zeroed")
            for i, v in enumerate(VARIANTS):
                for f, _ in FIELDS:
                    want_all = per[0]["steps"][step]["oracle"][i][f]
                    for r, p in enumerate(per):
                        if p["n_atmos"] == 0:
                            continue
                        got = p["steps"][step]["out"][i][f]
                        w = want_all[p["atmos_offset"]: p["atmos_offset"] + p["n_atmos"]]
                        edge = np.zeros(p["n_atmos"], bool)
                        edge[0] = p["left"] >= 0
                        edge[-1] = edge[-1] or p["right"] >= 0
                        same = _bits(got) == _bits(w)
                        shared += int(edge.sum())
                        if not same[~edge].all():
                            problems.append(f"{name} {v} {f} rank {r} step {step}: interior differs")
                        if special == "off":
                            differing += int((~same & edge).sum())
                        elif not same[edge].all():
                            problems.append(f"{name} {v} {f} rank {r} step {step}: a shared cell differs from the "
                                            "one-rank engine")
        if shared == 0:
            problems.append(f"{name}: no shared boundary cell exercised")
        if special == "off" and differing == 0:
            problems.append(f"{name}: with the option off no shared cell differed (the control shows nothing)")
        if special == "tiny_middle" and not (per[1]["n_atmos"] == 1 and per[1]["left"] == per[1]["right"] >= 0
                                             and per[1]["left_pos"] > 0 and per[2]["left_pos"] > per[1]["left_pos"]):
            problems.append(f"{name}: middle rank should hold one cell with one slot, got {per[1]}")
        if special == "empty_middle" and not (per[1]["n_atmos"] == 0 and per[2]["left_pos"] > 0):
            problems.append(f"{name}: expected an empty middle rank, got {per[1]}")
    assert not problems, "\n".join(problems[:40])
