"""The multi-GPU forms of a training step (one process per GPU), of which engine.NAFEngine picks one in its constructor: two
data-parallel exchanges that follow the engine's bucketed backward (AllReduceExchange, ShardedExchange) and a step of its own
(LevelParallelStep).  Each owns its streams, events and timing (bench.py); the exchange arithmetic is in dist.py.
"""
from __future__ import annotations

import contextlib
import ctypes

import torch
import torch.distributed as dist

from . import _abi
from . import dist as naf_dist
from . import fused


def _event(device):
    """An event recorded once, so that torch has created its hipEvent_t and the handle can be handed to the library."""
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(device))
    return ev


def _mark(stream):
    """A timing event recorded on `stream` now (comm_timing)."""
    ev = torch.cuda.Event(enable_timing=True)
    ev.record(stream)
    return ev


class _Route:
    """What every form offers the engine: train_step, gather_state, timing(enable) and report()."""
    time, timings = False, ()

    def timing(self, enable):
        self.time, self.timings = bool(enable), []

    def gather_state(self):
        """Nothing to do where every rank holds the complete table and moments."""


class _DataParallel(_Route):
    """Bucket setup of both data-parallel forms.  Buckets = level ranges in the order the scatter finishes them (dist.default_bucket_levels;
    `points_per_step`, this rank's sample points per step when known, picks the single-range exchange for small steps)."""

    def __init__(self, eng, bucket_levels, points_per_step):
        if bucket_levels is None:
            bucket_levels = naf_dist.default_bucket_levels(eng.net.encoder.num_levels, points_per_step)
        self.levels = [(int(a), int(b)) for a, b in bucket_levels]
        if len(self.levels) > _abi.MAX_GRAD_BUCKETS:
            raise ValueError(f"at most {_abi.MAX_GRAD_BUCKETS} gradient buckets")
        self.eng = eng
        self.comm = torch.cuda.Stream(device=eng.device)
        self.ready = [_event(eng.device) for _ in self.levels]
        self.mlp_ready, self.mlp_done = _event(eng.device), _event(eng.device)
        self.slices = naf_dist.grad_bucket_slices(eng.offsets.tolist(), eng.net.encoder.level_dim, self.levels)
        self.mlp_slice = (eng._emb_flat.numel(), eng.grad_flat.numel())                # MLP gradient + loss cell
        self.struct = st = _abi.GradBuckets(n_buckets=len(self.levels), mlp_ready=self.mlp_ready.cuda_event)
        for i, (a, b) in enumerate(self.levels):
            st.level_begin[i], st.level_end[i] = a, b
            st.ready[i] = self.ready[i].cuda_event

    def __getitem__(self, key):                          # bench.py reads engine._dp["levels"]
        return getattr(self, key)

    @contextlib.contextmanager
    def _span(self, stream, spans):
        """With timing on, a pair of timing events on `stream` around what the body issues."""
        t0 = _mark(stream) if self.time else None
        yield
        if self.time:
            spans.append((t0, _mark(stream)))

    def train_step(self, rays, target, weight, t_rand, ray_base, rays_all=None, global_ray_base=None):
        self.eng.backward(rays, target, weight, t_rand, ray_base)
        self.exchange_and_step()

    def report(self):
        """-> {"allreduce_ms_per_step": time the collectives were in flight on the side stream (sum over buckets), "tail_ms_per_step":
        time the main stream spent from the end of its own compute to the end of its last Adam launch}.  Synchronises."""
        if not self.timings:
            return None
        torch.cuda.synchronize(self.eng.device)
        steps = self.timings
        in_flight = sum(sum(a.elapsed_time(b) for a, b in spans) for spans, _, _, _ in steps) / len(steps)
        tail = sum(c0.elapsed_time(c1) for _, c0, _, c1 in steps) / len(steps)
        return {"allreduce_ms_per_step": in_flight, "tail_ms_per_step": tail}


class AllReduceExchange(_DataParallel):
    """All-reduce with replicated Adam.  On the side stream, per bucket in the order the scatter finishes them: wait for the
    bucket's event, all-reduce its slice of the flat gradient buffer.  On the main stream: as each sum arrives, Adam on exactly
    that slice of the parameters (so the last exchange overlaps the first bucket's update)."""

    def __init__(self, eng, bucket_levels, points_per_step):
        super().__init__(eng, bucket_levels, points_per_step)
        self.done = [_event(eng.device) for _ in self.levels]
        self.update_slices = naf_dist.aligned_update_slices(self.slices)             # Adam works on 16-byte groups

    def exchange_and_step(self):
        e, comm, timing = self.eng, self.comm, self.time
        main = torch.cuda.current_stream(e.device)
        spans = []
        order = [(self.mlp_ready, self.mlp_done, self.mlp_slice)] + list(zip(self.ready, self.done, self.slices))
        with torch.cuda.stream(comm):
            for ready, done, (a, b) in order:
                comm.wait_event(ready)
                with self._span(comm, spans):
                    dist.all_reduce(e.grad_flat[a:b], group=e.process_group)
                    done.record(comm)
        c0 = _mark(main) if timing else None                # end of this rank's own compute
        e.step_count += 1
        emb, m, v, g = (t.view(-1) for t in (e.emb, e.emb_m, e.emb_v, e.emb_g))
        lp = None if e.emb_lp is None else e.emb_lp.view(-1)
        waited = []
        for done, (a, b) in zip(self.done, self.update_slices):
            main.wait_event(done)
            if timing:
                waited.append(_mark(main))
            e._adam(emb[a:b], m[a:b], v[a:b], g[a:b], None if lp is None else lp[a:b], e._lp_code, "adam_step(table bucket)")
        main.wait_event(self.mlp_done)
        e._adam(e.mlp, e.mlp_m, e.mlp_v, e.mlp_g, None, 0, "adam_step(mlp)")
        if timing:
            self.timings.append((spans, c0, waited, _mark(main)))


class ShardedExchange(_DataParallel):
    """A sharded optimiser (ZeRO-1 style).  Per bucket, in the order the scatter finishes them:
    reduce-scatter of its gradient range on the side stream (each rank receives the SUM over ranks of its 1/N shard) -> Adam on
    exactly that shard of parameter and moments on the main stream -> all-gather of the updated shard of the table the kernels read
    (the 16-bit shadow in 16-bit mode).  The fp32 master of the shards other ranks own is refreshed only on demand (`gather_state`,
    before an evaluation or a checkpoint).  The MLP gradient + loss (17 KB) are all-reduced and stepped on every rank."""

    def __init__(self, eng, bucket_levels, points_per_step):
        super().__init__(eng, bucket_levels, points_per_step)
        # exchange ranges are multiples of world * 4 elements (boundaries moved in favour of the bucket that finishes later, the
        # table's end extended into the buffer's padding), so every rank owns an equal, 16-byte-aligned shard of each
        ranges = naf_dist.sharded_exchange_slices(self.slices, eng.world, eng._emb_flat.numel())
        self.shards = [(a, b, *naf_dist.shard_bounds(a, b, eng.world, eng.rank, eng.emb.numel())) for a, b in ranges]    # a, b, lo, end, hi
        longest = max(end - lo for _, _, lo, end, _ in self.shards)
        self.shard_grad = [torch.zeros(longest, device=eng.device) for _ in self.levels]       # reduce-scatter outputs
        self.rs_done = [_event(eng.device) for _ in self.levels]
        self.adam_done = [_event(eng.device) for _ in self.levels]
        self.gathered = _event(eng.device)

    def exchange_and_step(self):
        e, comm, timing, grp = self.eng, self.comm, self.time, self.eng.process_group
        main = torch.cuda.current_stream(e.device)
        spans = []
        with torch.cuda.stream(comm):
            comm.wait_event(self.mlp_ready)
            a, b = self.mlp_slice
            with self._span(comm, spans):
                dist.all_reduce(e.grad_flat[a:b], group=grp)
                self.mlp_done.record(comm)
            for i, (a, b, lo, end, _) in enumerate(self.shards):
                comm.wait_event(self.ready[i])
                with self._span(comm, spans):
                    dist.reduce_scatter_tensor(self.shard_grad[i][:end - lo], e.grad_flat[a:b], group=grp)
                    e.grad_flat[a:b].zero_()                 # the next step's scatter accumulates from zero
                    self.rs_done[i].record(comm)
        c0 = _mark(main) if timing else None                # end of this rank's own compute
        e.step_count += 1
        emb, m, v = (t.view(-1) for t in (e.emb, e.emb_m, e.emb_v))
        read_flat = e._emb_flat if e._lp_flat is None else e._lp_flat      # what the kernels gather from
        waited = []
        for i, (_, _, lo, _, hi) in enumerate(self.shards):
            main.wait_event(self.rs_done[i])
            if timing:
                waited.append(_mark(main))
            if hi > lo:
                lp = None if e._lp_flat is None else e._lp_flat[lo:hi]
                e._adam(emb[lo:hi], m[lo:hi], v[lo:hi], self.shard_grad[i][:hi - lo], lp, e._lp_code, "adam_step(table shard)")
            self.adam_done[i].record(main)
        main.wait_event(self.mlp_done)
        e._adam(e.mlp, e.mlp_m, e.mlp_v, e.mlp_g, None, 0, "adam_step(mlp)")
        with torch.cuda.stream(comm):
            for i, (a, b, lo, end, _) in enumerate(self.shards):
                comm.wait_event(self.adam_done[i])
                with self._span(comm, spans):
                    mine = read_flat[lo:end].clone()         # out of place: no aliasing assumptions on the backend
                    dist.all_gather_into_tensor(read_flat[a:b], mine, group=grp)
            self.gathered.record(comm)
        main.wait_event(self.gathered)                       # the next forward reads the gathered table
        if timing:
            self.timings.append((spans, c0, waited, _mark(main)))

    def gather_state(self):
        """Collective: every rank ends up with the complete fp32 master (16-bit mode) and Adam moments."""
        e = self.eng
        if e.world == 1:
            return
        torch.cuda.current_stream(e.device).wait_event(self.gathered)
        n_emb = e.emb.numel()
        full = [e.emb_m.view(-1), e.emb_v.view(-1)] + ([e.emb.view(-1)] if e._lp_flat is not None else [])
        for a, b, lo, end, hi in self.shards:
            for t in full:
                mine = torch.zeros(end - lo, device=e.device)
                mine[:hi - lo] = t[lo:hi]
                out = torch.empty(b - a, device=e.device)
                dist.all_gather_into_tensor(out, mine, group=e.process_group)
                t[a:min(b, n_emb)] = out[:min(b, n_emb) - a]


class LevelParallelStep(_Route):
    """Rank k owns the levels [k L/N, (k+1) L/N): their rows of the table, of the 16-bit shadow and of the Adam moments are
    current on that rank only (`gather_state` completes them everywhere before an evaluation or a checkpoint)."""
    PHASES = ("encode_ms", "features_all_to_all_ms", "field_ms", "gradients_all_to_all_ms", "scatter_adam_ms")

    def __init__(self, eng, rays_hint):
        L, N = eng.net.encoder.num_levels, eng.world
        if L % N != 0:
            raise ValueError(f"dp_mode 'levels' needs a world size that divides the {L} levels (got {N}); use 'sharded'")
        per = L // N
        # with one or two levels per rank the scatter uses 256 row buckets per level instead of 64 (NAF_CFG_MIN_BUCKETS): 256 / 512 reducer
        # workgroups that each own their rows, so that no launch is split and the reducer applies Adam itself (tools/levels_emulate.py,
        # 8 ranks: reduce + Adam 0.102 -> 0.064 ms per step; with four levels per rank 128 buckets measured no gain: 0.270 against 0.261 ms)
        eng._levels_flags = {1: 2, 2: 2}.get(per, 0) << _abi.CFG_MIN_BUCKETS_SHIFT
        offs = [int(v) for v in eng.offsets.tolist()]
        C = eng.net.encoder.level_dim
        self.eng, self.rays_hint = eng, rays_hint
        self.levels = (eng.rank * per, (eng.rank + 1) * per)
        self.rows = [(offs[k * per] * C, offs[(k + 1) * per] * C) for k in range(N)]      # element ranges by owner
        self.comm = torch.cuda.Stream(device=eng.device)
        self.mlp_ready, self.mlp_done, self.grads_ready = _event(eng.device), _event(eng.device), _event(eng.device)
        self.exchange = torch.cuda.Stream(device=eng.device)
        self.n = None                                        # rays per rank and step, fixed by the first step
        self.bufs = None                                     # send, feat, dfeat, recv

    def _all_to_all(self, out, inp):
        """Equal-split all-to-all of two contiguous device buffers (RCCL; the gloo rehearsal of a one-GPU box stages through the host)."""
        grp = self.eng.process_group
        if dist.get_backend(grp) == "gloo" and inp.is_cuda:
            o = torch.empty(out.shape, dtype=out.dtype)
            dist.all_to_all_single(o.view(torch.uint8).view(-1), inp.cpu().view(torch.uint8).view(-1), group=grp)
            out.copy_(o)
        else:
            dist.all_to_all_single(out.view(-1), inp.view(-1), group=grp)

    def train_step(self, rays, target, weight, t_rand, ray_base, rays_all=None, global_ray_base=None):
        """One level-parallel step (include/naf_hip.h, naf_levels_*): encode the owned levels for every rank's points -> all-to-all
        -> MLP forward / loss / backward on the own rays -> all-to-all of the feature gradients (+ a 17 KB all-reduce of the MLP
        gradient and the loss behind it, overlapping the scatter) -> scatter + Adam on the owned levels.  Same result as the
        data-parallel step and as one process on the concatenated batch.  Every rank must bring the same number of rays; the jitter
        index of ray j of rank k is global_ray_base + k * n + j; `global_ray_base` defaults to ray_base - rank * n (the convention
        ray_base = (step * world + rank) * n of trainer.py / bench.py) -- a caller with another convention passes it explicitly (the
        same value on every rank).  `rays_all` [world * n, 8]: all ranks' rays in rank order when the caller has them (a shared
        pixel draw); otherwise they are all-gathered (32 KB per rank)."""
        e = self.eng
        N, r, grp = e.world, e.rank, e.process_group
        n, S = rays.shape[0], e.n_samples
        L, C = e.net.encoder.num_levels, e.net.encoder.level_dim
        lb, le = self.levels
        nl = le - lb
        if n == 0:
            raise ValueError("dp_mode 'levels': every rank needs the same, non-zero number of rays per step")
        main = torch.cuda.current_stream(e.device)
        if self.n is None:
            # The first step fixes the batch size of the run.  Every rank has its first step at the same time, so the cross-rank check
            # below is issued by ALL ranks or by none (a per-size cache would let one rank skip a collective another rank issues --
            # mismatched collectives, i.e. a hang until the group's timeout); with a rays_per_step_hint (the YAML's n_rays / world:
            # trainer.py, bench.py) the size is validated locally and no collective is needed at all.
            if self.rays_hint is not None:
                if n != self.rays_hint:
                    raise ValueError(f"dp_mode 'levels': this rank brought {n} rays, the engine was built for {self.rays_hint} per rank "
                                     f"and step (rays_per_step_hint); use dp_mode 'sharded' for uneven shards")
            else:
                both = torch.tensor([n, -n], device=e.device, dtype=torch.int64)
                dist.all_reduce(both, op=dist.ReduceOp.MAX, group=grp)
                if int(both[0]) != n or int(both[1]) != -n:
                    raise ValueError(f"dp_mode 'levels': ranks hold different numbers of rays this step (this rank {n}, largest {int(both[0])}, "
                                     f"smallest {-int(both[1])}); use dp_mode 'sharded' for uneven shards")
            self.n = n
        elif n != self.n:
            raise ValueError(f"dp_mode 'levels': {n} rays in this step, {self.n} in the first one -- a level-parallel run keeps one batch "
                             f"size per rank (equal-split collectives); use dp_mode 'sharded' for varying or uneven shards")
        if rays_all is None:
            rays_all = torch.empty(N * n, 8, device=e.device)
            dist.all_gather_into_tensor(rays_all, rays.contiguous(), group=grp)
        elif rays_all.shape[0] != N * n:
            raise ValueError("rays_all must hold world_size * n rays")
        t_all = None
        if t_rand is not None:
            t_all = torch.empty(N * n, t_rand.shape[1], device=e.device)
            dist.all_gather_into_tensor(t_all, t_rand.contiguous(), group=grp)
        fdt = torch.float32 if int(e.mlp_precision) == _abi.F32 else torch.bfloat16
        run = n * S * C                                            # elements of one (rank, level)
        if self.bufs is None:                                      # n is fixed from here on
            mk = lambda *shape: torch.empty(*shape, dtype=fdt, device=e.device)
            self.bufs = (mk(N, nl, run), mk(L, run), mk(L, run), mk(N, nl * run))
        send, feat, dfeat, recv = self.bufs
        e._grow_acc(n)
        g_base = (ray_base - r * n) if global_ray_base is None else int(global_ray_base)
        cfg_all, cfg = e._cfg(g_base & 0xffffffff), e._cfg((g_base + r * n) & 0xffffffff)
        ws = fused.workspace(cfg_all, N * n * S, e.device)
        lib, sp = _abi.lib(), _abi.stream_ptr()
        marks = []

        def mark():
            if self.time:
                marks.append(_mark(main))
        mark()
        _abi.check(lib.naf_levels_encode(_abi.ptr(rays_all), _abi.ptr(t_all), _abi.ptr(e.table), _abi.ptr(e.offsets), _abi.ptr(send),
                                         N * n, N, ctypes.byref(cfg_all), lb, le, sp), "levels_encode")      # one block per destination rank
        mark()
        self._all_to_all(feat, send)                                # block k of the result = rank k's levels of MY points: [L][points][C]
        mark()
        _abi.check(lib.naf_levels_field_step(_abi.ptr(rays), _abi.ptr(t_rand), _abi.ptr(target), _abi.ptr(weight), _abi.ptr(feat),
                                             _abi.ptr(e.mlp), _abi.ptr(e.acc), _abi.ptr(dfeat), _abi.ptr(e.mlp_g),
                                             _abi.ptr(e.loss), n, ctypes.byref(cfg), _abi.ptr(ws), self.grads_ready.cuda_event, sp),
                   "levels_field_step")
        self.mlp_ready.record(main)
        mark()
        # the gradients' all-to-all starts behind the MLP backward kernel (the event), not behind the slab reduction that follows it
        ex = self.exchange
        ex.wait_event(self.grads_ready)
        with torch.cuda.stream(ex):
            self._all_to_all(recv, dfeat)                           # block k = rank k's gradients of MY levels
        main.wait_stream(ex)
        mark()
        with torch.cuda.stream(self.comm):                          # issued after the all-to-all, so it queues behind it on the links
            self.comm.wait_event(self.mlp_ready)
            dist.all_reduce(e.grad_flat[e._emb_flat.numel():], group=grp)      # MLP gradient + loss
            e.step_count += 1
            e._adam(e.mlp, e.mlp_m, e.mlp_v, e.mlp_g, None, 0, "adam_step(mlp)")      # beside the scatter, not behind it
            self.mlp_done.record(self.comm)
        st = e._table_adam()
        applied = ctypes.c_int(0)
        _abi.check(lib.naf_levels_scatter(_abi.ptr(rays_all), _abi.ptr(t_all), _abi.ptr(recv), nl * run * fdt.itemsize, N, _abi.ptr(e.offsets),
                                          _abi.ptr(e.emb_g), N * n, ctypes.byref(cfg_all), lb, le, _abi.ptr(ws), ctypes.byref(st),
                                          ctypes.byref(applied), sp), "levels_scatter")
        if not applied.value:
            # the reducer launches were split (few levels per rank) or the batch took the atomic scatter: the gradient of the owned
            # rows sits in emb_g
            e._adam_rows(*self.rows[r], what="adam_step(owned levels)")
        main.wait_event(self.mlp_done)                              # the next step reads the stepped MLP
        mark()
        if self.time:
            self.timings.append(marks)
        fused._bump(e.device)

    def gather_state(self):
        """Collective: every owner broadcasts its rows of the master table, the moments and the 16-bit shadow."""
        e = self.eng
        if e.world == 1:
            return
        flats = [e.emb.view(-1), e.emb_m.view(-1), e.emb_v.view(-1)] + ([] if e.emb_lp is None else [e.emb_lp.view(-1)])
        for k, (a, b) in enumerate(self.rows):
            for t in flats:
                dist.broadcast(t[a:b], src=dist.get_global_rank(e.process_group, k), group=e.process_group)

    def report(self):
        """-> mean ms per step of each of PHASES, and the two all-to-alls as "allreduce_ms_per_step" / "tail_ms_per_step".  Synchronises."""
        if not self.timings:
            return None
        torch.cuda.synchronize(self.eng.device)
        steps = self.timings
        out = {k: sum(m[i].elapsed_time(m[i + 1]) for m in steps) / len(steps) for i, k in enumerate(self.PHASES)}
        out["allreduce_ms_per_step"] = out["features_all_to_all_ms"] + out["gradients_all_to_all_ms"]
        out["tail_ms_per_step"] = out["allreduce_ms_per_step"]
        return out
