"""Multi-GPU plumbing: one process per GPU, `torch.distributed` (backend "nccl" = RCCL on ROCm,
"gloo" on CPU for tests).  Inference and voting shard by IMAGE with no exchange on the data
path: ranks are independent replicas; the only collectives are the benchmark's
barrier and its max-over-ranks clock.  Training is data-parallel: `StepExchange` is the exchange
of one step (SyncBN tables, bucketed gradient all-reduces) and its accounting.
"""
from __future__ import annotations

import math
import os
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch
import torch.distributed as dist


def force_collectives() -> bool:
    """CASAPOSE_DIST_FORCE=1: create the process group and run every collective of the data-parallel protocol even with ONE rank, so that
    the RCCL code path (group creation, barrier with device ids, fp64 statistic all-reduces, asynchronous gradient buckets on RCCL's
    stream) executes on a single-GPU box.  A SUM over one rank is the identity: results must equal the plain single-process run."""
    return os.environ.get("CASAPOSE_DIST_FORCE", "0") == "1"


def init_from_env(backend: str = "nccl") -> Tuple[int, int, int]:
    """Reads RANK / LOCAL_RANK / WORLD_SIZE (torchrun contract); returns (rank, local_rank, world)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # CASAPOSE_DIST_BACKEND=gloo lets several ranks share ONE GPU in tests (RCCL refuses duplicate devices)
    backend = os.environ.get("CASAPOSE_DIST_BACKEND", backend)
    if (world > 1 or force_collectives()) and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        dist.init_process_group(backend, rank=rank, world_size=world)
    return rank, local, world


def shard_range(total: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous [begin, end) slice of `total` images for `rank`; sizes differ by at most one and
    the union over ranks is exactly range(total) (ragged tails included)."""
    if world < 1 or not (0 <= rank < world):
        raise ValueError("bad rank/world: %d/%d" % (rank, world))
    base, extra = divmod(total, world)
    begin = rank * base + min(rank, extra)
    return begin, begin + base + (1 if rank < extra else 0)


def barrier_sync(device=None) -> None:
    if dist.is_initialized():
        if dist.get_backend() == "nccl" and device is not None and torch.device(device).type == "cuda":
            dist.barrier(device_ids=[torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()])
        else:
            dist.barrier()
    if device is not None and torch.device(device).type == "cuda":
        torch.cuda.synchronize(device)


def max_over_ranks(value: float, device=None) -> float:
    if not dist.is_initialized():
        return float(value)
    t = torch.tensor([value], dtype=torch.float64, device=device if device is not None else "cpu")
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def sum_over_ranks(value: float, device=None) -> float:
    if not dist.is_initialized():
        return float(value)
    t = torch.tensor([value], dtype=torch.float64, device=device if device is not None else "cpu")
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return float(t.item())


def all_reduce_sum_(t: torch.Tensor, group=None, world_size: int = 1) -> torch.Tensor:
    """In-place SUM all-reduce (RCCL on GPU tensors, gloo on CPU tensors); no-op for a single replica.  The training
    step uses it for (a) the fp64 SyncBN statistic tables -- forward sums and the two backward means -- and (b) the
    flat fp32 gradient before Adam (MirroredStrategy's SUM reduction, train_casapose.py:641-643)."""
    if world_size > 1 or (force_collectives() and dist.is_initialized()):
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    return t


def all_reduce_sum_async(t: torch.Tensor, group=None):
    """Start a SUM all-reduce of `t` and return the work handle (`.wait()` makes the current stream wait for it).  RCCL runs it on its
    own stream after the work already queued on the current stream, so it overlaps whatever is launched next."""
    return dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group, async_op=True)


def reduce_step_log(losses, pose_stats, world_size: int, device=None):
    """The per-step logging exchange of the training driver as ONE collective: `losses` (5 python floats) become their MEAN over the
    replicas (strategy.reduce(MEAN), train_casapose.py:690-694), `pose_stats` (a sequence of >= 6 per-object vectors, or None) its first
    six vectors SUMMED over the replicas (:732-737).  Returns (list of floats, [6, objects] float64 array or None)."""
    import numpy as np

    st = None if pose_stats is None else np.stack([np.asarray(pose_stats[j], np.float64).reshape(-1) for j in range(6)])
    if world_size <= 1 or not dist.is_initialized():
        return [float(v) for v in losses], st
    flat = np.concatenate([np.asarray(losses, np.float64) / world_size] + ([st.reshape(-1)] if st is not None else []))
    t = torch.from_numpy(flat).to(device if device is not None and dist.get_backend() == "nccl" else "cpu")
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    flat = t.cpu().numpy()
    n = len(losses)
    return [float(v) for v in flat[:n]], (flat[n:].reshape(st.shape) if st is not None else None)


def gradient_buckets(offsets: Dict[str, Tuple[int, Tuple[int, ...]]], size: int, op_keys: Sequence[Sequence[str]], order: Sequence[str],
                     starts: Sequence[str]) -> List[Tuple[int, int, int]]:
    """[(first op index, start, end)] of the contiguous slices of the flat gradient (`offsets` / `size`: ParamStore's layout, every parameter
    padded to a multiple of four floats) that are final once the backward has executed the op `first op index` (ops run in reverse;
    `op_keys[i]` = the parameter keys op i completes).  A bucket starts at each layer of `starts` that is in the forward `order`:
    decoder 2 | decoder 1 | stage 4 | the rest of the encoder."""
    rank = {n: i for i, n in enumerate(order)}
    cuts = sorted(rank[b] for b in starts if b in rank)

    def bucket_of(key):
        r = rank.get(key.split(".")[0], len(rank))
        return max([i for i, s0 in enumerate(cuts) if r >= s0] + [0])

    nb = len(cuts)
    lo, hi, first = [size] * nb, [0] * nb, [len(op_keys)] * nb
    for name, (off, shape) in offsets.items():
        b, n = bucket_of(name), math.prod(shape)
        lo[b], hi[b] = min(lo[b], off), max(hi[b], off + n + ((-n) % 4))
    for i, keys in enumerate(op_keys):
        for k in keys:
            b = bucket_of(k)
            first[b] = min(first[b], i)
    out = [(first[b], lo[b], hi[b]) for b in range(nb) if hi[b] > lo[b]]
    covered = sorted((a, e) for _, a, e in out)
    assert covered[0][0] == 0 and covered[-1][1] == size and all(covered[i][1] == covered[i + 1][0] for i in range(len(covered) - 1)), \
        "gradient buckets must tile the flat buffer"
    return out


def _between_events(collective: Callable[[], None]):
    """Run `collective` between two timing events recorded on the current stream; returns the pair."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    collective()
    e1.record()
    return e0, e1


class StepExchange:
    """The data-parallel exchange of one training step over the flat gradient `grad`, and its accounting.  Three ordering rules:
    a bucket's SUM all-reduce goes out (asynchronously, on the collective library's stream) immediately after the backward op that
    completes it, so the exchange of the decoders' gradients overlaps the encoder's backward; `before_send(stream, a, e)` has taken this
    replica's OWN loss factor out of grad[a:e] before the slice is summed; nobody waits for a handle before wait().
    `plan_buckets()` -> [(first op index, start, end)] (gradient_buckets) is called on the first backward that needs buckets.

    log (start_log): every exchange point of a step in launch order -- ("step_begin",), ("syncbn", bytes, "blocking", "compute") for a
    statistic table all-reduce (the next kernel needs it), ("op", index) for every backward op, ("grad_bucket", bytes, "async", stream id of
    the compute stream at launch, first op index) where a bucket's all-reduce is launched, ("grad_wait", n) where the compute stream waits
    for the buckets.  Recorded with or without replicas (a single replica launches no collective but passes the same points), so that the
    overlap can be asserted structurally (tests/test_gpu_dp.py, tests/test_distributed_cpu.py) and counted (bench.py --mode train).
    timing (start_timing): event pairs on the compute stream around every collective the step WAITS for; report() sums them."""

    def __init__(self, grad: torch.Tensor, group, world_size: int, plan_buckets: Callable[[], List[Tuple[int, int, int]]],
                 before_send: Callable[[int, int, int], None]):
        self.grad, self.group, self.world_size = grad, group, world_size
        self.plan_buckets, self.before_send = plan_buckets, before_send
        self.log: Optional[list] = None      # start_log()
        self.timing: Optional[dict] = None   # start_timing()
        self.buckets: Optional[List[Tuple[int, int, int]]] = None
        self.pending: list = []              # handles of the bucket all-reduces in flight
        self.running = False                 # collectives really run in this backward (begin_backward)

    def _bracket(self, key: str, collective: Callable[[], None]) -> bool:
        """Run `collective`; with timing on (and a group) between two events on the current stream, kept under timing[key]."""
        if self.timing is None or self.group is None:
            collective()
            return False
        self.timing[key].append(_between_events(collective))
        return True

    def begin_step(self):
        if self.log is not None:
            self.log.append(("step_begin",))

    def reduce_stats(self, table: torch.Tensor):
        """SUM a SyncBN statistic table over the replicas (blocking: the next kernel reads it)."""
        if self.log is not None:
            self.log.append(("syncbn", table.numel() * table.element_size(), "blocking", "compute"))
        self._bracket("syncbn", lambda: all_reduce_sum_(table, self.group, self.world_size))

    def begin_backward(self) -> bool:
        """Returns whether this backward's collectives really run (with replicas, or forced at one rank)."""
        self.pending = []
        self.running = self.group is not None and (self.world_size > 1 or force_collectives())
        if (self.running or self.log is not None) and self.buckets is None:
            self.buckets = self.plan_buckets()
        return self.running

    def _launch(self, stream: int, due: Callable[[int, int], bool]):
        if not self.running and self.log is None:
            return
        for first, a, e in self.buckets:
            if due(first, a):
                if self.log is not None:
                    self.log.append(("grad_bucket", 4 * (e - a), "async", stream, first))
                if self.running:
                    self.before_send(stream, a, e)   # (the loss factor is this replica's own: out before the sum over replicas)
                    self.pending.append(all_reduce_sum_async(self.grad[a:e], self.group))

    def after_op(self, i: int, stream: int):
        """Backward op `i` has been launched on `stream`: send the buckets it completes (the one at offset 0 waits for finish_backward)."""
        if self.log is not None:
            self.log.append(("op", i))
        self._launch(stream, lambda first, a: first == i and a != 0)

    def finish_backward(self, stream: int):
        """The whole tape and the plan's fix-ups of the first parameters are launched: send the bucket that starts at offset 0."""
        self._launch(stream, lambda first, a: a == 0)

    def wait(self):
        """Complete the exchange started by the backward (or run it as one blocking all-reduce if nothing is pending)."""
        if self._bracket("grad_wait", self._drain):
            self.timing["steps"] += 1

    def _drain(self):
        if self.log is not None:
            self.log.append(("grad_wait", len(self.pending)))
        if self.pending:
            for h in self.pending:
                h.wait()
            self.pending = []
        else:
            all_reduce_sum_(self.grad, self.group, self.world_size)

    def start_log(self):
        self.log = []

    def structure(self) -> dict:
        """Per step, from the log of the LAST logged step: blocking collectives (SyncBN tables) and their payload, gradient buckets, their payload and
        how many backward ops are launched AFTER each bucket's all-reduce (what its exchange can hide behind)."""
        log = self.log or []
        last = len(log) - 1 - next((i for i, e in enumerate(reversed(log)) if e[0] == "step_begin"), len(log) - 1)
        step = log[last + 1:] if log and log[last][0] == "step_begin" else log
        bn = [e for e in step if e[0] == "syncbn"]
        buckets, after = [], []
        for i, e in enumerate(step):
            if e[0] == "grad_bucket":
                buckets.append(e)
                after.append(sum(1 for x in step[i + 1:] if x[0] == "op"))
        return {"blocking_collectives_per_step": len(bn), "blocking_payload_bytes_per_step": int(sum(e[1] for e in bn)),
                "gradient_buckets": len(buckets), "gradient_payload_bytes_per_step": int(sum(e[1] for e in buckets)),
                "backward_ops_launched_after_each_bucket": after, "backward_ops": sum(1 for e in step if e[0] == "op"),
                "note": "structure of the data-parallel step, identical for every world size: the blocking calls sit on the critical path (global-batch "
                        "statistics, as the reference's SyncBatchNormalization), each gradient bucket's all-reduce is launched asynchronously when the "
                        "backward has passed the bucket's first layer"}

    def start_timing(self):
        """From the next step on, bracket the SyncBN table all-reduces (blocking: the next kernel needs the global statistics) and the wait
        for the gradient buckets (whatever of their exchange the backward did not cover); no host synchronisation inside a step."""
        self.timing = {"syncbn": [], "grad_wait": [], "steps": 0}

    def report(self) -> dict:
        """{"syncbn_ms", "syncbn_calls", "grad_wait_ms", "exposed_ms", "grad_total_ms", "grad_hidden_ms", "grad_bytes"} per step.  exposed =
        time the compute stream spent inside / waiting for collectives; grad_total = the same gradient buckets all-reduced back to back on an
        idle GPU (measured here, after the steps), so grad_hidden = grad_total - grad_wait is what the overlap with the backward bought."""
        t = self.timing
        torch.cuda.synchronize(self.grad.device)
        steps = max(t["steps"], 1)
        bn = sum(a.elapsed_time(b) for a, b in t["syncbn"]) / steps
        gw = sum(a.elapsed_time(b) for a, b in t["grad_wait"]) / steps
        total, nbytes = 0.0, 0
        if self.group is not None and self.buckets:
            scratch = torch.zeros_like(self.grad)

            def back_to_back():
                for h in [all_reduce_sum_async(scratch[a:e], self.group) for _, a, e in self.buckets]:
                    h.wait()

            for rep in range(3):
                e0, e1 = _between_events(back_to_back)
                e1.synchronize()
                total = e0.elapsed_time(e1)   # the last repetition (the first pays RCCL's lazy set-up)
            nbytes = 4 * scratch.numel()
        return {"syncbn_ms": round(bn, 4), "syncbn_calls": len(t["syncbn"]) // steps, "grad_wait_ms": round(gw, 4), "exposed_ms": round(bn + gw, 4),
                "grad_total_ms": round(total, 4), "grad_hidden_ms": round(max(total - gw, 0.0), 4), "grad_bytes": nbytes}
