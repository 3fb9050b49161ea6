"""world_size-2 gloo test of the N>1 plumbing used by bench.py (image sharding, barrier,
max-over-ranks clock).  Runs on CPU."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from casapose_amd import parallel

    r, l, w = parallel.init_from_env("gloo")
    assert (r, w) == (rank, world)
    b, e = parallel.shard_range(37, r, w)
    parallel.barrier_sync()
    mx = parallel.max_over_ranks(1.0 + rank)          # the slowest rank's clock
    total = parallel.sum_over_ranks(float(e - b))     # images processed by all ranks
    q.put((rank, b, e, mx, total))
    torch.distributed.destroy_process_group()


def test_two_rank_sharding_and_clock():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (r0, b0, e0, m0, t0), (r1, b1, e1, m1, t1) = res
    assert (b0, e0, b1, e1) == (0, 19, 19, 37)   # ragged split, union = range(37)
    assert m0 == m1 == 2.0 and t0 == t1 == 37.0


def test_shard_range_properties():
    from casapose_amd.parallel import shard_range

    for total in (0, 1, 7, 16, 257):
        for world in (1, 2, 3, 8):
            spans = [shard_range(total, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == total
            assert all(spans[i][1] == spans[i + 1][0] for i in range(world - 1))
            sizes = [e - b for b, e in spans]
            assert max(sizes) - min(sizes) <= 1
    with pytest.raises(ValueError):
        shard_range(4, 2, 2)


def _syncbn_worker(rank, world, port, q):
    """The SyncBN protocol of the training step on CPU tensors: every rank holds half of the batch, all-reduces
    the fp64 statistic tables exactly as TrainPlan does, and must reproduce the whole-batch normalisation and its
    gradient (compared with the autograd oracle on the full batch)."""
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import numpy as np

    from casapose_amd import parallel

    parallel.init_from_env("gloo")
    rng = np.random.default_rng(0)                      # same data on both ranks; each takes its shard
    n, c = 64, 8
    x = torch.from_numpy(rng.standard_normal((n, c)) * 2 + 1)
    dy = torch.from_numpy(rng.standard_normal((n, c)))
    gamma = torch.from_numpy(1 + 0.1 * rng.standard_normal(c))
    b, e = parallel.shard_range(n, rank, world)
    xl, dyl = x[b:e], dy[b:e]
    eps = 2e-5
    sums = torch.cat([xl.sum(0), (xl * xl).sum(0)])    # cp_bn_stats_f32
    parallel.all_reduce_sum_(sums, None, world)
    N = (e - b) * world
    mean = sums[:c] / N
    var = sums[c:] / N - mean * mean
    rstd = torch.rsqrt(var + eps)
    xh = (xl - mean) * rstd
    g = dyl * gamma
    chan = torch.cat([g.sum(0), (g * xh).sum(0)])       # cp_bn_act_bwd_reduce_f32 (chan table)
    parallel.all_reduce_sum_(chan, None, world)
    dx = rstd * (g - chan[:c] / N - xh * chan[c:] / N)  # cp_bn_act_bwd_apply_f32
    grad = torch.cat([(dyl * xh).sum(0)])               # d gamma, local part
    parallel.all_reduce_sum_(grad, None, world)         # the flat-gradient all-reduce
    q.put((rank, b, e, mean.numpy(), var.numpy(), dx.numpy(), grad.numpy()))
    torch.distributed.destroy_process_group()


def test_two_rank_syncbn_protocol_matches_whole_batch():
    import numpy as np

    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_syncbn_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=120) for _ in range(world)), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    rng = np.random.default_rng(0)
    n, c = 64, 8
    x = torch.tensor(rng.standard_normal((n, c)) * 2 + 1, requires_grad=True)
    dy = torch.from_numpy(rng.standard_normal((n, c)))
    gamma = torch.tensor(1 + 0.1 * rng.standard_normal(c), requires_grad=True)
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    y = (x - mean) / torch.sqrt(var + 2e-5) * gamma
    y.backward(dy)
    dx = np.concatenate([r[5] for r in res])
    assert np.allclose(res[0][3], mean.detach().numpy(), atol=1e-12) and np.allclose(res[1][4], var.detach().numpy(), atol=1e-10)
    assert np.allclose(dx, x.grad.numpy(), atol=1e-10)
    assert np.allclose(res[0][6], gamma.grad.numpy(), atol=1e-10) and np.allclose(res[1][6], gamma.grad.numpy(), atol=1e-10)


def _log_worker(rank, world, port, q):
    import numpy as np

    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from casapose_amd import parallel
    from casapose_amd.data_handler.synthetic_scene import SyntheticSceneDataset

    parallel.init_from_env("gloo")
    calls = {"n": 0}
    real = torch.distributed.all_reduce

    def counting(*a, **k):
        calls["n"] += 1
        return real(*a, **k)

    torch.distributed.all_reduce = counting
    losses = [1.0 + rank, 2.0 * rank, 0.5, 3.0, rank * rank]
    stats = [np.arange(8, dtype=np.float64) * (j + 1) + rank for j in range(8)]
    mean, st = parallel.reduce_step_log(losses, stats, world, None)
    mean2, st2 = parallel.reduce_step_log(losses, None, world, None)
    torch.distributed.all_reduce = real
    # every replica renders only its slice of the GLOBAL batch (ragged: 7 images over 3 replicas), and the slices partition it
    ds = SyntheticSceneDataset(3, (64, 64), length=7, seed=5, random_crop=False)
    it, n = ds.generate_dataset(7, 1, shard=(rank, world))
    mine = next(it)
    q.put((rank, mean, st, mean2, st2 is None, calls["n"], mine["img"].numpy(), n))
    torch.distributed.destroy_process_group()


def test_three_rank_packed_logging_and_source_sharding():
    """ONE collective per step for the logged quantities (5 losses as MEAN, 6 pose-statistic vectors as SUM; train_casapose.py:690-694,
    732-737) and per-replica data sharding at the source, world size 3 with a ragged global batch."""
    import numpy as np

    from casapose_amd.data_handler.synthetic_scene import SyntheticSceneDataset

    world = 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_log_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=180) for _ in range(world)), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want_mean = [np.mean([1.0 + r for r in range(3)]), np.mean([2.0 * r for r in range(3)]), 0.5, 3.0, np.mean([r * r for r in range(3)])]
    want_st = np.stack([sum(np.arange(8, dtype=np.float64) * (j + 1) + r for r in range(3)) for j in range(6)])
    whole = SyntheticSceneDataset(3, (64, 64), length=7, seed=5, random_crop=False).batch(0, 7)["img"].numpy()
    got = np.concatenate([r[6] for r in res])
    assert [r[6].shape[0] for r in res] == [3, 2, 2] and np.array_equal(got, whole)
    for rank, mean, st, mean2, none2, ncalls, _, n in res:
        assert np.allclose(mean, want_mean) and np.allclose(mean2, want_mean) and np.allclose(st, want_st) and none2
        assert ncalls == 2 and n == 1                     # exactly one all-reduce per logged step


# --------------------------------------------------------------------------------------------------
# the data-parallel exchange of a training step (parallel.StepExchange) without a GPU or the shared library
# --------------------------------------------------------------------------------------------------
def test_gradient_buckets_tile_the_real_parameter_layout():
    """Four buckets (decoder 2 | decoder 1 | stage 4 | the rest) over the flat buffer of the real network: contiguous, 16-byte aligned,
    each one final after an EARLIER op than the bucket behind it (the backward runs the ops in reverse), whatever the order of the dict."""
    import random

    import casapose_oracle as O
    import numpy as np

    from casapose_amd.parallel import gradient_buckets
    from casapose_amd.train_engine import BUCKET_STARTS, ParamStore, forward_order

    st = ParamStore(O.init_params(4, 27, seed=1, dtype=np.float32), torch.device("cpu"))
    order = forward_order()
    op_keys = [[k for k in st.offsets if k.split(".")[0] == layer] for layer in order]   # one op per layer
    buckets = gradient_buckets(st.offsets, st.size, op_keys, order, BUCKET_STARTS)
    by_offset = sorted(buckets, key=lambda b: b[1])
    assert len(buckets) == 4
    assert by_offset[0][1] == 0 and by_offset[-1][2] == st.size and all(by_offset[i][2] == by_offset[i + 1][1] for i in range(3))
    assert all(a % 4 == 0 and e % 4 == 0 and e > a for _, a, e in buckets)
    assert by_offset[0][0] == 0
    firsts = [f for f, _, _ in by_offset]
    assert all(firsts[i] < firsts[i + 1] for i in range(3))
    items = list(st.offsets.items())
    for shuffled in (items[::-1], random.Random(3).sample(items, len(items))):
        assert gradient_buckets(dict(shuffled), st.size, op_keys, order, BUCKET_STARTS) == buckets


_EX_BUCKETS = [(0, 0, 16), (2, 16, 28), (5, 28, 48), (6, 48, 64)]   # (first op, start, end) over eight ops; the backward runs 7..0
_EX_KINDS = (["step_begin", "syncbn"] + ["op", "op", "grad_bucket", "op", "grad_bucket", "op", "op", "op", "grad_bucket", "op", "op", "grad_bucket"]
             + ["grad_wait"])


def _drive_exchange(ex, table):
    """One step as TrainPlan.train_step / backward() drive it."""
    ex.start_log()
    ex.begin_step()
    ex.reduce_stats(table)
    running = ex.begin_backward()
    for i in range(7, -1, -1):
        ex.after_op(i, 0)
    ex.finish_backward(0)
    ex.wait()
    return running


def _exchange_integers(rank):
    import numpy as np

    return torch.from_numpy(np.random.default_rng(10 + rank).integers(-8, 9, 64).astype(np.float32))


def _exchange_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from casapose_amd import parallel

    parallel.init_from_env("gloo")
    factor = 2.0 ** (3 + rank)                           # every replica's OWN loss factor
    grad = _exchange_integers(rank) * factor
    sent, waits = [], []

    def before_send(stream, a, e):
        sent.append((a, e, len(ex.pending)))
        grad[a:e] /= factor

    real_async = parallel.all_reduce_sum_async

    class _Spy:
        def __init__(self, h):
            self.h = h

        def wait(self):
            waits.append(len(ex.log))
            return self.h.wait()

    parallel.all_reduce_sum_async = lambda t, group=None: _Spy(real_async(t, group))
    ex = parallel.StepExchange(grad, torch.distributed.group.WORLD, world, lambda: list(_EX_BUCKETS), before_send)
    table = torch.full((6,), 1.0 + rank, dtype=torch.float64)
    running = _drive_exchange(ex, table)
    q.put((rank, running, grad.numpy(), table.numpy(), list(ex.log), len(ex.pending), ex.structure(), sent, waits))
    torch.distributed.destroy_process_group()


def test_two_rank_step_exchange_protocol():
    """Each bucket goes out right after the op that completes it, with the replica's own power-of-two factor already out of the slice;
    nobody waits for a handle before wait(); afterwards both replicas hold the exact sum (small integers: no rounding anywhere)."""
    import numpy as np

    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_exchange_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=120) for _ in range(world)), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = (_exchange_integers(0) + _exchange_integers(1)).numpy()
    for rank, running, grad, table, log, npending, st, sent, waits in res:
        assert running
        assert np.array_equal(grad, want) and np.array_equal(table, np.full(6, 3.0))
        assert npending == 0
        assert [e[0] for e in log] == _EX_KINDS and log[1] == ("syncbn", 48, "blocking", "compute") and log[-1] == ("grad_wait", 4)
        bidx = [i for i, e in enumerate(log) if e[0] == "grad_bucket"]
        assert len(waits) == 4 and all(w == len(log) for w in waits)       # every handle is waited for after ("grad_wait", 4), the last entry
        assert [log[i] for i in bidx] == [("grad_bucket", 4 * (e - a), "async", 0, first) for first, a, e in reversed(_EX_BUCKETS)]
        assert all(log[i - 1] == ("op", log[i][4]) for i in bidx)          # directly behind the op that completes it; offset 0 behind ("op", 0), last
        assert log[bidx[-1]][4] == 0 and bidx[-1] == len(log) - 2
        assert sent == [(a, e, k) for k, (_, a, e) in enumerate(reversed(_EX_BUCKETS))]   # the factor leaves a slice once, before its own send
        assert st["backward_ops_launched_after_each_bucket"] == [6, 5, 2, 0] and st["backward_ops"] == 8
        assert st["gradient_buckets"] == 4 and st["gradient_payload_bytes_per_step"] == 4 * 64
        assert st["blocking_collectives_per_step"] == 1 and st["blocking_payload_bytes_per_step"] == 48


def test_step_exchange_without_a_group_sends_nothing_and_logs_the_same_structure(monkeypatch):
    """The structure of a step is identical for every world size (bench.py prints it from a single-replica run): the same log entries,
    no collective, and the loss factor is left to the plan's single-replica unscale."""
    from casapose_amd import parallel

    def refuse(*a, **k):
        raise AssertionError("a single replica starts no collective")

    monkeypatch.setattr(parallel, "all_reduce_sum_async", refuse)
    monkeypatch.setattr(torch.distributed, "all_reduce", refuse)
    grad = _exchange_integers(0) * 8.0
    before = grad.clone()
    table = torch.full((6,), 1.0, dtype=torch.float64)
    ex = parallel.StepExchange(grad, None, 1, lambda: list(_EX_BUCKETS), refuse)
    assert not _drive_exchange(ex, table)
    assert torch.equal(grad, before) and torch.equal(table, torch.full((6,), 1.0, dtype=torch.float64)) and not ex.pending
    assert [e[0] for e in ex.log] == _EX_KINDS and ex.log[-1] == ("grad_wait", 0)
    st = ex.structure()
    assert st["backward_ops_launched_after_each_bucket"] == [6, 5, 2, 0] and st["gradient_payload_bytes_per_step"] == 4 * 64
