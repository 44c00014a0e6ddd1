"""One-process-per-GPU data parallelism for the hot path.

Frames are independent through the whole path, so ranks process disjoint frames and the data path
has NO collective.  The only cross-rank traffic the reference has on this path is the reduction of
the loss/log scalars (`reduce_dict`, CP/det3d/torchie/trainer/utils.py:157-183; `all_reduce`,
VR/pcdet/utils/commu_utils.py:148-162) and the timing/barrier protocol of the benchmark.  Backend
"nccl" is RCCL on ROCm (xGMI inside a node); "gloo" is used by the CPU tests.
"""
import os
import socket
import subprocess
import sys

import torch
import torch.distributed as dist


def free_port():
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_ranks(nprocs, script, argv, master_port=None, env=None, timeout=None):
    """Run `script argv...` as `nprocs` ranks of ONE node, one process per GPU, the way the reference launches its
    trainers (`python -m torch.distributed.launch --nproc_per_node=N tools/train.py`, CP/docs/GETTING_START.md;
    the worker side is CP/det3d/torchie/apis/train.py:289-295): torch.distributed.run with a 127.0.0.1 rendezvous
    exports RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* to every rank, which `init_from_env` reads.  Returns the exit
    code of the launcher (0 only when every rank exited cleanly)."""
    port = int(master_port) if master_port else free_port()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(int(nprocs)),
           "--master-addr", "127.0.0.1", "--master-port", str(port), script] + list(argv)
    e = dict(os.environ if env is None else env)
    e.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: RCCL needs it on this driver
    e.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 1) // max(1, int(nprocs)))))
    return subprocess.call(cmd, env=e, timeout=timeout)


def init_from_env(backend=None, single=False):
    """Reads RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT (torch.distributed.run).
    Returns (rank, local_rank, world_size).  A single process stays without a process group unless `single` is set (or
    the launcher exported WORLD_SIZE=1 explicitly): then a one-rank group is created, so that the collectives of the step
    run through the backend (RCCL) at N = 1 exactly as they do at N > 1."""
    launched = "WORLD_SIZE" in os.environ
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if (world > 1 or single or launched) and not dist.is_initialized():
        if backend is None:
            backend = "nccl" if torch.cuda.is_available() else "gloo"
        if world > 1:
            # several ranks: ALWAYS the launcher's rendezvous.  A private one-rank group here would leave every rank
            # believing it is alone while frame_shard() still divides the frames by `world`.
            missing = [k for k in ("MASTER_ADDR", "MASTER_PORT") if k not in os.environ]
            if missing:
                raise RuntimeError("init_from_env: WORLD_SIZE=%d but %s not set (launch with torch.distributed.run "
                                   "--master-addr 127.0.0.1 --master-port P)" % (world, " / ".join(missing)))
            dist.init_process_group(backend, init_method="env://")
        elif launched and "MASTER_PORT" in os.environ:
            dist.init_process_group(backend, init_method="env://")
        else:
            dist.init_process_group(backend, init_method="tcp://127.0.0.1:%d" % free_port(), rank=0, world_size=1)
    if dist.is_initialized() and dist.get_world_size() != world:
        raise RuntimeError("init_from_env: process group has %d ranks, WORLD_SIZE says %d"
                           % (dist.get_world_size(), world))
    return rank, local, world


def is_dist():
    """A process group exists (any world size: a one-rank RCCL group still runs its collectives)."""
    return dist.is_available() and dist.is_initialized()


def frame_shard(num_frames, rank, world):
    """DistributedSampler-style frame assignment without padding: frame i goes to rank i % world."""
    return list(range(rank, num_frames, world))


def barrier(device=None):
    if is_dist():
        dist.barrier()
    if torch.cuda.is_available():
        torch.cuda.synchronize(device)


def max_over_ranks(value, device="cpu"):
    """Elapsed time of the slowest rank (the driver contract: barrier, time, MAX over ranks)."""
    if not is_dist():
        return float(value)
    t = torch.tensor([float(value)], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def reduce_dict(input_dict, average=True):
    """CP/det3d/torchie/trainer/utils.py:157-183: the values of the (sorted-key) dict go through ONE reduce to
    rank 0, which averages them; the other ranks get the un-divided partial result back, like the reference.
    The reference stacks scalars; here the values are flattened into one buffer, so per-task vectors (`CenterHead`
    returns one value per task) and entries of different shapes travel in the same single collective."""
    if not is_dist():
        return input_dict
    world = dist.get_world_size()
    with torch.no_grad():
        names = sorted(input_dict.keys())
        parts = [input_dict[k].reshape(-1) for k in names]
        values = torch.cat(parts) if len(parts) > 1 else parts[0].clone()
        dist.reduce(values, dst=0)
        if dist.get_rank() == 0 and average:
            values /= world
        out, pos = {}, 0
        for k, p in zip(names, parts):
            out[k] = values[pos:pos + p.numel()].view(input_dict[k].shape)
            pos += p.numel()
        return out


def _collective_device():
    """Device the collective buffers live on: the current GPU under RCCL, the host under gloo."""
    return torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")


def all_gather(data):
    """CP/det3d/torchie/trainer/utils.py:114-157: all_gather of an arbitrary picklable object -> list over ranks (the
    evaluation loop's `all_predictions = all_gather(detections)`, trainer.py:471).  Same protocol -- the sizes first, then
    the pickles padded to the longest -- as two collectives of ONE tensor each (`all_gather_into_tensor`) instead of
    2 x world_size one-element tensors."""
    import pickle
    if not is_dist() or dist.get_world_size() == 1:
        return [data]
    world = dist.get_world_size()
    dev = _collective_device()
    buf = torch.frombuffer(bytearray(pickle.dumps(data)), dtype=torch.uint8).to(dev)
    sizes = torch.zeros(world, dtype=torch.int64, device=dev)
    dist.all_gather_into_tensor(sizes, torch.tensor([buf.numel()], dtype=torch.int64, device=dev))
    sizes = sizes.tolist()
    cap = max(sizes)
    padded = torch.zeros(cap, dtype=torch.uint8, device=dev)
    padded[:buf.numel()] = buf
    out = torch.empty(world * cap, dtype=torch.uint8, device=dev)
    dist.all_gather_into_tensor(out, padded)
    host = out.cpu().numpy()
    return [pickle.loads(host[r * cap:r * cap + sizes[r]].tobytes()) for r in range(world)]


def gather_detections(frame_ids, boxes, scores, labels, counts):
    """Detections of every rank on every rank without pickling: the fixed-capacity device tensors the detection tails
    produce (`CenterHead.predict_device`, `TransFusionHead.get_bboxes`: boxes [F, cap, D], scores / labels [F, cap], counts [F]
    for this rank's F frames, `frame_ids` [F] = their global indices) travel as ONE packed fp32 buffer through one
    `all_gather_into_tensor` -- F may differ between ranks (7 frames over 2 ranks), so the frame counts go first.
    -> {frame id: dict(box3d_lidar, scores, label_preds)} over all ranks, the merge `predictions.update(p)` of the
    reference's evaluation loop (trainer.py:471-480)."""
    F, cap, D = boxes.shape
    pack = torch.cat([torch.as_tensor(frame_ids, device=boxes.device).reshape(F, 1).float(), counts.reshape(F, 1).float(),
                      scores.reshape(F, cap).float(), labels.reshape(F, cap).float(), boxes.reshape(F, cap * D).float()], 1)
    width = pack.shape[1]
    if not is_dist() or dist.get_world_size() == 1:
        allp, nf = pack, [F]
    else:
        world = dist.get_world_size()
        dev = _collective_device()
        nfr = torch.zeros(world, dtype=torch.int64, device=dev)
        dist.all_gather_into_tensor(nfr, torch.tensor([F], dtype=torch.int64, device=dev))
        nf = nfr.tolist()
        fmax = max(nf)
        mine = torch.zeros((fmax, width), dtype=torch.float32, device=dev)
        mine[:F] = pack.to(dev)
        got = torch.empty((world * fmax, width), dtype=torch.float32, device=dev)
        dist.all_gather_into_tensor(got, mine)
        allp = torch.cat([got[r * fmax:r * fmax + nf[r]] for r in range(world)])
    out = {}
    host = allp.cpu()
    for row in host:
        fid, k = int(row[0]), int(row[1])
        out[fid] = dict(scores=row[2:2 + k].clone(), label_preds=row[2 + cap:2 + cap + k].long(),
                        box3d_lidar=row[2 + 2 * cap:].reshape(cap, D)[:k].clone())
    return out


def all_reduce_value(data, op="sum", average=False):
    """VR/pcdet/utils/commu_utils.py:148-162."""
    if not is_dist():
        return data
    ops = {"SUM": dist.ReduceOp.SUM, "MAX": dist.ReduceOp.MAX, "MIN": dist.ReduceOp.MIN,
           "PRODUCT": dist.ReduceOp.PRODUCT}
    out = data.clone()
    dist.all_reduce(out, op=ops[op.upper()])
    if average:
        assert op.upper() == "SUM"
        return out / dist.get_world_size()
    return out


# ---------------------------------------------------------------------------------------------------------------
# Gradient reduction of the data-parallel training step
def allreduce_grads(params, coalesce=True, bucket_size_mb=-1):
    """The reference's synchronous gradient average (CP/det3d/core/utils/dist_utils.py:8-42, called by its
    DistOptimizerHook after `loss.backward()`): all-reduce every `param.grad`, divided by the world size -- coalesced
    into flat buffers (one per dtype, or buckets of `bucket_size_mb`) or tensor by tensor."""
    grads = [p.grad.data for p in params if p.requires_grad and p.grad is not None]
    if not is_dist() or not grads:
        return
    world = dist.get_world_size()
    if not coalesce:
        for g in grads:
            dist.all_reduce(g.div_(world))
        return
    buckets = {}
    if bucket_size_mb > 0:
        limit, cur, size = bucket_size_mb * 1024 * 1024, [], 0
        out = []
        for g in grads:
            if cur and (size + g.numel() * g.element_size() > limit or g.dtype != cur[0].dtype):
                out.append(cur)
                cur, size = [], 0
            cur.append(g)
            size += g.numel() * g.element_size()
        if cur:
            out.append(cur)
        groups = out
    else:
        for g in grads:
            buckets.setdefault(g.dtype, []).append(g)
        groups = list(buckets.values())
    for group in groups:
        flat = torch.cat([g.reshape(-1) for g in group])
        dist.all_reduce(flat)
        flat.div_(world)
        pos = 0
        for g in group:
            g.copy_(flat[pos:pos + g.numel()].view_as(g))
            pos += g.numel()


class GradBucketReducer(object):
    """Bucketed gradient all-reduce overlapped with backward -- what `DistributedDataParallel` does for the reference
    (CP/det3d/torchie/apis/train.py:289-295), laid out for one MI355X node: xGMI is point-to-point (a ring all-reduce is
    bound by one ~150 GB/s link), so the gradients travel in FEW LARGE buckets (default 16 MB: the 35.8 MB of the
    CenterPoint detector are three, so the first two travel while backward still runs), and the buckets are the
    gradients' own storage:

      * every parameter owns a view into one flat buffer per bucket (parameters in reverse registration order = the order
        backward produces them).  `zero_grad()` sets the gradients to None, so autograd ASSIGNS each produced gradient (no
        `grad += new` kernel per parameter: ~400 small launches and 1.7 ms of a 36 ms CenterPoint + fusion step, measured);
        when a bucket is complete its gradients move into the flat buffer in ONE multi-tensor copy and `.grad` becomes the
        view -- after `finish()` the optimizer reads the reduced gradients in place, no copy-back pass (the reference's
        coalesced path copies every gradient twice, one launch each);
      * a post-accumulate-grad hook counts a bucket's finished gradients; a complete bucket is launched asynchronously
        (RCCL runs it on its own stream while backward continues) -- STRICTLY IN BUCKET ORDER: bucket i only once buckets
        0..i-1 are launched, otherwise it waits for them or for `finish()`.  Every rank therefore issues the same sequence
        of collectives even when the set of parameters that received a gradient differs between ranks (a data-dependent
        branch), which is what DDP guarantees with its fixed bucket order;
      * `finish()` waits for the outstanding buckets and scales by 1 / world size (folded into the all-reduce for
        backends with an AVG op).

    Parameters that received no gradient in a step (unused branches) keep zeros in the bucket, like
    `find_unused_parameters=True`; their bucket is launched by `finish()`."""

    def __init__(self, params, bucket_mb=16.0):
        self.params = [p for p in params if p.requires_grad]
        self.world = dist.get_world_size() if is_dist() else 1
        self._group = is_dist()
        self.buckets = []            # dict(flat, params, pending, handle)
        limit = int(bucket_mb * 1024 * 1024)
        cur, size = [], 0
        for p in reversed(self.params):
            nbytes = p.numel() * p.element_size()
            if cur and (size + nbytes > limit or p.dtype != cur[0].dtype or p.device != cur[0].device):
                self._seal(cur)
                cur, size = [], 0
            cur.append(p)
            size += nbytes
        if cur:
            self._seal(cur)
        self._hooks = [p.register_post_accumulate_grad_hook(self._on_grad) for p in self.params]
        self._next = 0               # buckets [0, _next) are launched

    def _seal(self, plist):
        flat = torch.zeros(sum(p.numel() for p in plist), dtype=plist[0].dtype, device=plist[0].device)
        pos = 0
        offsets, views = {}, []
        for p in plist:
            views.append(flat[pos:pos + p.numel()].view_as(p))
            p.grad = views[-1]
            offsets[id(p)] = pos
            pos += p.numel()
        b = dict(flat=flat, params=plist, pending=len(plist), handle=None, index=len(self.buckets), offsets=offsets,
                 views=views)
        for p in plist:
            p._df3d_bucket = b
        self.buckets.append(b)

    def _launch_ready(self, force=False):
        """Launch buckets in index order while they are complete (all of them with `force`)."""
        while self._next < len(self.buckets):
            b = self.buckets[self._next]
            if b["pending"] > 0 and not force:
                return
            self._next += 1
            self._collect(b)
            if self._group:
                b["handle"] = dist.all_reduce(b["flat"], op=dist.ReduceOp.SUM, async_op=True)

    @staticmethod
    def _collect(b):
        """The bucket's gradients -> its flat buffer (one multi-tensor copy; zeros for parameters without a gradient), `.grad` ->
        the views.  A gradient that already IS its view (accumulated in place: a caller that did not use zero_grad()) stays."""
        dst, src, zero = [], [], []
        for p, view in zip(b["params"], b["views"]):
            g = p.grad
            if g is None:
                zero.append(view)
            elif g.data_ptr() != view.data_ptr():
                dst.append(view)
                src.append(g)
            p.grad = view
        with torch.no_grad():
            if dst:
                torch._foreach_copy_(dst, src)
            if zero:
                torch._foreach_zero_(zero)

    def _on_grad(self, p):
        b = p._df3d_bucket
        b["pending"] -= 1
        if b["pending"] == 0:
            self._launch_ready()

    @staticmethod
    def _offset(b, p):
        """Byte offset of the parameter's gradient view inside its bucket (looked up, not searched: the hooks and
        zero_grad call this for every parameter every step)."""
        try:
            return b["offsets"][id(p)] * p.element_size()
        except KeyError:
            raise KeyError("parameter not in bucket")

    def _view(self, b, p):
        off = self._offset(b, p) // p.element_size()
        return b["flat"][off:off + p.numel()].view_as(p)

    def zero_grad(self):
        """Start a step: every gradient None (autograd then assigns what backward produces; the buckets are filled -- and
        zeroed where a parameter got no gradient -- when they are launched).  Use INSTEAD of optimizer.zero_grad()."""
        for b in self.buckets:
            b["pending"] = len(b["params"])
            b["handle"] = None
            for p in b["params"]:
                p.grad = None
        self._next = 0

    def finish(self):
        """After backward: launch what is left (buckets with unused parameters), wait, average."""
        self._launch_ready(force=True)
        for b in self.buckets:
            if b["handle"] is not None:
                b["handle"].wait()
                b["handle"] = None
            if self.world > 1:
                b["flat"].div_(self.world)

    def remove(self):
        for h in self._hooks:
            h.remove()
        self._hooks = []


class BucketAdamW(object):
    """AdamW (TF/configs/transfusion_nusc_voxel_F.py:302: `optimizer = dict(type='AdamW', lr=..., weight_decay=0.01)`) over the
    buckets of a `GradBucketReducer` instead of over ~400 parameter tensors: every parameter is re-seated as a view of ONE flat
    buffer per bucket (same offsets as its gradient view), the optimizer state is two flat buffers per bucket, and a step is one
    fused launch per bucket on contiguous memory (the multi-tensor kernel over the individual tensors took 0.8 ms of the
    27 ms cp_fusion step: 28 chunked launches).  Same arithmetic as `torch.optim.AdamW` element by element.
    Parameters without a gradient in a step see the zeros the reducer keeps for them (what DistributedDataParallel hands the
    optimizer for unused parameters): their moments decay and weight decay applies.
    The views keep their own version counters, which an in-place update of the flat buffer does not move; `step()` bumps them
    (host side) so that every weight pack of the library (`derived.tensors_key`) sees the update.
    Re-seating happens once, here: move / cast the model BEFORE building the reducer and this optimizer."""

    def __init__(self, reducer, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        self.reducer = reducer
        self.flat = []
        with torch.no_grad():
            for b in reducer.buckets:
                fp = torch.empty_like(b["flat"])
                for p in b["params"]:
                    off = b["offsets"][id(p)]
                    v = fp[off:off + p.numel()].view(p.shape)
                    v.copy_(p.detach())
                    p.data = v
                P = torch.nn.Parameter(fp, requires_grad=True)
                P.grad = b["flat"]
                self.flat.append(P)
        on_gpu = bool(self.flat) and self.flat[0].is_cuda
        self.inner = torch.optim.AdamW(self.flat, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, fused=on_gpu or None)

    @property
    def param_groups(self):
        return self.inner.param_groups

    def clip_grad_norm(self, max_norm, norm_type=2):
        """mmcv `OptimizerHook.clip_grads` over the flat gradient buffers (after `reducer.finish()`): one norm per bucket."""
        return torch.nn.utils.clip_grad_norm_(self.flat, max_norm=max_norm, norm_type=norm_type,
                                              foreach=(bool(self.flat) and self.flat[0].is_cuda) or None)

    def step(self):
        for P, b in zip(self.flat, self.reducer.buckets):
            P.grad = b["flat"]
        self.inner.step()
        torch.autograd.graph.increment_version(self.reducer.params)

    def zero_grad(self, set_to_none=True):
        self.reducer.zero_grad()

