"""The non-finite guard with two ranks (beside tests/test_gpu_exchange_ranks.py, through the mock
RCCL of tests/cpp/mock_rccl.cpp): with FCX_OPT_CHECK_FINITE on and a NaN in rank 1's inputs only,
both ranks complete their collective -- every rank queues its all-reduce before it reads its
verdict -- the mock's call logs are those of the same run with the check off, and rank 1 alone
reports."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_gpu_exchange_ranks import FIELDS, MOCK, _uid  # noqa: E402

N = 24_012  # the APPLE cut of 2 ranks falls inside an atmosphere cell
CELL = 4097  # of rank 1's shard


def _run(rank, world, uid, check, log):
    import torch
    from fcx import _lib
    from fcx.basic import PHASE_ALL, PHASE_NORMAL
    from fcx.comm import Comm
    from fcx.engine import Engine
    from fcx.parallel import apple_range, local_atmos, synthetic_atmos_map
    from fcx.synthetic import build_case
    from test_gpu_multirank import shard_case

    os.environ["FCX_MOCK_RCCL_LOG"] = log
    amap = synthetic_atmos_map(N)
    ranges = [apple_range(N, r, world) for r in range(world)]
    la = local_atmos(amap, rank, world, ranges=ranges)
    off, size = ranges[rank]
    comm = Comm(0, world, rank, uid)
    case = shard_case(build_case("CCLM", n=N, T=1, bias=True, seed=41), off, off + size, "CCLM", seed=41)
    if rank == 1:
        case.lf.field[(1, 1, "TATM")][CELL] = np.nan
    outs = {f: torch.full((la.n_atmos,), float("nan"), dtype=torch.float64, device="cuda:0") for f, _ in FIELDS}
    atmos = {"local": la, "fields": [(PHASE_NORMAL, 1, g, f, outs[f]) for f, g in FIELDS],
             "own_boundaries": True, "comm": comm}
    eng = Engine(case.lf, 1, case.methods, corrections=case.corrections, atmos=atmos,
                 options={"check_finite": check})
    rec = {"shared": (la.left >= 0) + (la.right >= 0), "errors": []}
    try:
        eng.upload(PHASE_ALL)
        for step in range(2):
            try:
                eng.run(PHASE_ALL, 3600 * step)
                rec["errors"].append(None)
            except _lib.NonFiniteError as ex:
                rec["errors"].append((ex.name, ex.cell, bool(np.isnan(ex.value)), ex.is_atmos))
        torch.cuda.synchronize()
        rec["out"] = {f: outs[f].cpu().numpy() for f, _ in FIELDS}
    finally:
        eng.close()
        comm.close()
    return rec


def _child(rank, world, uids, logdir, q):
    os.environ["FCX_RCCL_LIBRARY"] = MOCK
    os.environ["FCX_MOCK_RCCL_TIMEOUT_S"] = "30"
    try:
        import torch

        torch.cuda.set_device(0)
        q.put((rank, None, {check: _run(rank, world, uid, check, os.path.join(logdir, f"check{check}"))
                            for check, uid in zip((0, 3), uids)}))
    except Exception as ex:  # noqa: BLE001 -- reported to the parent
        import traceback

        q.put((rank, traceback.format_exc() + repr(ex), None))


def test_a_rank_that_finds_a_nan_completes_its_collective(tmp_path):
    import torch.multiprocessing as mp

    assert os.path.exists(MOCK)
    world = 2
    uids = [_uid(), _uid()]
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    procs = [ctx.Process(target=_child, args=(r, world, uids, str(tmp_path), q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(world):
        rank, err, out = q.get()
        assert err is None, f"rank {rank}: {err}"
        res[rank] = out
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    logs = {c: [open(os.path.join(tmp_path, f"check{c}.{r}")).read() for r in range(world)] for c in (0, 3)}
    assert logs[0][0] == logs[0][1] and logs[0][0].count("\n") >= 2  # an all-reduce per step
    assert logs[3] == logs[0]  # the check changes no rank's collective sequence
    assert res[0][0]["shared"] + res[1][0]["shared"] > 0
    assert res[0][0]["errors"] == res[1][0]["errors"] == res[0][3]["errors"] == [None, None]
    assert res[1][3]["errors"] == [("TATM", CELL, True, False)] * 2  # rank 1 alone reports, every step
    for r in range(world):  # ... and the check changes no value, the shared cell's included
        for f, _ in FIELDS:
            assert res[r][3]["out"][f].tobytes() == res[r][0]["out"][f].tobytes(), (r, f)
