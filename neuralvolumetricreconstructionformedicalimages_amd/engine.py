"""Training engine for the fused hot path: one `naf_render_train` + two `naf_adam_step` launches per step.

Replaces, for the canonical NAF network, what reference src/trainer.py:134-142 + train.py:48-135 do per step
(6 chunks x ~40 ATen launches, per-chunk 57 MB zero-fill of the table gradient, dense torch.optim.Adam):
  * parameters, Adam moments and gradients are flat fp32 buffers that stay resident in HBM; the module's
    `encoder.embeddings` / `layers.i.weight|bias` are views of them, so state_dict() keeps the reference keys;
  * with a 16-bit table the fp32 master is updated by Adam and the bf16/fp16 shadow the kernels gather from is
    written in the same pass; the gradient buffer is zeroed in that pass too;
  * with a process group the constructor picks one multi-GPU form of the step (parallel.py): data parallel, where each bucket
    of levels' slice of the flat gradient buffer is exchanged (RCCL) on a side stream as soon as the bucketed backward has
    finished it, or level parallel.
"""
from __future__ import annotations

import ctypes

import torch

from . import _abi
from . import dist as naf_dist
from . import fused
from . import parallel


class NAFEngine:
    def __init__(self, net, n_samples, perturb=True, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, table_dtype=torch.float32,
                 mlp_precision=None, seed=0, process_group=None, n_streams=1, chunk_rays=16384, scatter_mode=None, cfg_flags=None,
                 bucket_levels=None, fuse_table_adam=True, dp_mode="sharded", rays_per_step_hint=None):
        if not net.fused_supported():
            raise RuntimeError("NAFEngine needs the canonical NAF network (in 32, hidden 32, 4 layers, skips=[2], out 1)")
        self.net = net
        enc = net.encoder
        dev = enc.embeddings.device
        if dev.type != "cuda":
            raise RuntimeError("NAFEngine: the network must live on the GPU (no CPU path)")
        self.device = dev
        self.n_samples, self.perturb = int(n_samples), bool(perturb)
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.seed = int(seed)
        self.step_count = 0
        self.rays_seen = 0
        self.process_group = process_group
        if dp_mode not in ("auto", "sharded", "allreduce", "levels"):
            raise ValueError("dp_mode must be 'sharded' (reduce-scatter, per-rank Adam on a table slice, all-gather), 'allreduce', "
                             "'levels' (each rank owns a range of levels; features and their gradients cross in two all-to-alls) or 'auto'")
        self.world, self.rank = 1, 0
        if process_group is not None:
            import torch.distributed as dist
            self.world, self.rank = dist.get_world_size(process_group), dist.get_rank(process_group)
        points_per_step = None if rays_per_step_hint is None else int(rays_per_step_hint) * self.n_samples
        if dp_mode == "auto":
            feat_bytes = 4 if (mlp_precision == _abi.F32 or (mlp_precision is None and table_dtype == torch.float32)) else 2
            dp_mode = naf_dist.pick_dp_mode(self.world, enc.num_levels, enc.level_dim, enc.embeddings.numel(), points_per_step, feat_bytes,
                                            4 if table_dtype == torch.float32 else 2)
        self.dp_mode = dp_mode
        self.scatter_mode, self.cfg_flags = scatter_mode, cfg_flags     # None: fused.scatter_mode() default (auto)
        # single-GPU, single-stream steps let the gradient reducer apply the table's Adam update itself (naf_render_train_adam:
        # the gradient table is neither written, re-read nor cleared; bit-identical to backward() + optimizer_step())
        self.fuse_table_adam = bool(fuse_table_adam)

        # ---- flat fp32 master parameters; module parameters become views ---------------------------------
        # The table lives in a flat buffer padded to dist.padded_length: the exchange ranges of a data-parallel step are multiples
        # of world * 4 elements (equal 16-byte-aligned shards per rank), the last one reaches into the padding.
        n_emb = enc.embeddings.numel()
        n_pad = naf_dist.padded_length(n_emb, self.world)
        self._emb_flat = torch.zeros(n_pad, device=dev)
        self._emb_flat[:n_emb] = enc.embeddings.data.float().reshape(-1)
        self.emb = self._emb_flat[:n_emb].view(enc.embeddings.shape)
        enc.embeddings.data = self.emb
        self.mlp = net.packed_mlp().detach().clone().contiguous()
        off = 0
        for lyr in net.layers:
            for p in (lyr.weight, lyr.bias):
                n = p.numel()
                p.data = self.mlp[off:off + n].view(p.shape)
                off += n
        assert off == _abi.MLP_PARAMS
        self.table_dtype = table_dtype
        self._lp_flat = None if table_dtype == torch.float32 else self._emb_flat.to(table_dtype)
        self.emb_lp = None if self._lp_flat is None else self._lp_flat[:n_emb].view(self.emb.shape)
        self._lp_code = 0 if self.emb_lp is None else _abi.dtype_code(table_dtype)       # the shadow's dtype for the Adam launches
        self.emb_m, self.emb_v = (torch.zeros_like(self.emb) for _ in range(2))
        self.mlp_m, self.mlp_v = (torch.zeros_like(self.mlp) for _ in range(2))
        # table gradient | MLP gradient | loss in ONE flat buffer (sections 256-byte aligned): a data-parallel step is a
        # single all-reduce
        n_mlp = self.mlp.numel()
        o_mlp = n_pad
        o_loss = o_mlp + (n_mlp + 63) // 64 * 64
        self.grad_flat = torch.zeros(o_loss + 64, device=dev)
        self.emb_g = self.grad_flat[:n_emb].view(self.emb.shape)
        self.mlp_g = self.grad_flat[o_mlp:o_mlp + n_mlp]
        self.loss = self.grad_flat[o_loss:o_loss + 1]
        self.acc = None
        self.offsets = enc.offsets.to(dev)
        enc.offsets = self.offsets
        self.mlp_precision = mlp_precision
        if mlp_precision is None:
            self.mlp_precision = _abi.F32 if table_dtype == torch.float32 else _abi.BF16
        # the multi-GPU form of the step (parallel.py), chosen once (None: single GPU); _dp: the data-parallel one, for the bucketed launch
        self._route = self._dp = None
        self._levels_flags = 0
        if process_group is not None:
            if int(n_streams) > 1:
                raise ValueError("NAFEngine: n_streams > 1 cannot be combined with a process group (the bucket events are "
                                 "recorded by the one launch that owns the gradient buffer)")
            if dp_mode == "levels":
                self._route = parallel.LevelParallelStep(self, None if rays_per_step_hint is None else int(rays_per_step_hint))
            else:
                exchange = parallel.ShardedExchange if dp_mode == "sharded" else parallel.AllReduceExchange
                self._route = self._dp = exchange(self, bucket_levels, points_per_step)
        # Optional multi-stream execution: the batch is cut into chunks that run their whole forward/backward pipeline on
        # alternating HIP streams, so the gather-bound, VALU-bound and store-bound kernels of different chunks overlap.
        # Each extra stream owns a gradient buffer, a workspace and a loss cell; they are summed before Adam.
        self.n_streams = max(1, int(n_streams))
        self.chunk_rays = int(chunk_rays)
        self._lanes = []
        for _ in range(self.n_streams - 1):
            self._lanes.append({"stream": torch.cuda.Stream(device=dev), "emb_g": torch.zeros_like(self.emb),
                                "mlp_g": torch.zeros_like(self.mlp), "loss": torch.zeros(1, device=dev), "ws": None})

    def broadcast_parameters(self, src=0):
        """Every rank starts from rank `src`'s table and MLP (and refreshes its 16-bit shadow)."""
        if self.process_group is None:
            return
        naf_dist.broadcast_parameters((self.emb, self.mlp), self.process_group, src)
        self.sync_from_module()

    # -------------------------------------------------------------------------------------------------------
    def _cfg(self, ray_base=0):
        enc = self.net.encoder
        return _abi.RenderCfg(n_samples=self.n_samples, perturb=int(self.perturb), bound=float(self.net.bound),
                              L=enc.num_levels, C=enc.level_dim, H=enc.base_resolution,
                              table_dtype=_abi.dtype_code(self.table_dtype), mlp_precision=int(self.mlp_precision),
                              last_activation=fused.LAST_ACTIVATIONS[self.net.last_activation],
                              seed=(self.seed + 0x9E3779B97F4A7C15 * (self.step_count + 1)) & (2 ** 64 - 1),
                              ray_index_base=int(ray_base), log2_hashmap_size=int(enc.log2_hashmap_size),
                              scatter_mode=fused._default_scatter_mode if self.scatter_mode is None else int(self.scatter_mode),
                              flags=(fused._default_flags if self.cfg_flags is None else int(self.cfg_flags)) | self._levels_flags)

    @property
    def table(self):
        return self.emb if self.emb_lp is None else self.emb_lp

    def _grow_acc(self, n):
        if self.acc is None or self.acc.numel() < n:
            self.acc = torch.empty(n, device=self.device)

    def _launch(self, rays, target, weight, t_rand, ray_base, acc, emb_g, mlp_g, loss, ws):
        n = rays.shape[0]
        cfg = self._cfg(ray_base)
        args = (_abi.ptr(rays), _abi.ptr(t_rand), _abi.ptr(target), _abi.ptr(weight), _abi.ptr(self.table), _abi.ptr(self.offsets),
                _abi.ptr(self.mlp), _abi.ptr(acc), _abi.ptr(emb_g), _abi.ptr(mlp_g), _abi.ptr(loss), n, ctypes.byref(cfg), _abi.ptr(ws))
        if self._dp is not None and emb_g is self.emb_g:
            _abi.check(_abi.lib().naf_render_train_bucketed(*args, ctypes.byref(self._dp.struct), _abi.stream_ptr()),
                       "render_train_bucketed")
        else:
            _abi.check(_abi.lib().naf_render_train(*args, _abi.stream_ptr()), "render_train")

    def backward(self, rays, target, weight, t_rand=None, ray_base=0):
        """Forward + weighted squared error + backward: fills the gradient buffers, returns acc [n]."""
        if isinstance(self._route, parallel.LevelParallelStep):
            raise NotImplementedError("dp_mode 'levels' has no separate backward / optimizer_step: a rank holds only its levels' rows "
                                      "(use train_step)")
        n = rays.shape[0]
        self._grow_acc(n)
        self.loss.zero_()
        if self.n_streams == 1 or n <= self.chunk_rays:
            cfg = self._cfg(ray_base)
            ws = fused.workspace(cfg, n * self.n_samples, self.device)
            self._launch(rays, target, weight, t_rand, ray_base, self.acc, self.emb_g, self.mlp_g, self.loss, ws)
            fused._bump(self.device)
            return self.acc[:n]
        return self._backward_multistream(rays, target, weight, t_rand, ray_base)

    def _backward_multistream(self, rays, target, weight, t_rand, ray_base):
        n, c = rays.shape[0], self.chunk_rays
        main = torch.cuda.current_stream()
        cfg = self._cfg(ray_base)
        need = int(_abi.lib().naf_render_workspace_bytes(ctypes.byref(cfg), c * self.n_samples))
        lanes = [{"stream": main, "emb_g": self.emb_g, "mlp_g": self.mlp_g, "loss": self.loss,
                  "ws": fused.workspace(cfg, c * self.n_samples, self.device)}] + self._lanes
        start = torch.cuda.Event()
        start.record(main)
        for lane in lanes[1:]:
            if lane["ws"] is None or lane["ws"].numel() < need:
                lane["ws"] = torch.empty(need, dtype=torch.uint8, device=self.device)
            lane["stream"].wait_event(start)                # inputs and parameters are ready
            with torch.cuda.stream(lane["stream"]):
                lane["loss"].zero_()
        for k, b in enumerate(range(0, n, c)):
            e = min(n, b + c)
            lane = lanes[k % len(lanes)]
            with torch.cuda.stream(lane["stream"]):
                tr = None if t_rand is None else t_rand[b:e]
                self._launch(rays[b:e], target[b:e], weight[b:e], tr, ray_base + b, self.acc[b:e], lane["emb_g"], lane["mlp_g"],
                             lane["loss"], lane["ws"])
        for lane in lanes[1:]:                              # fold the side streams' gradients into the main buffers
            done = torch.cuda.Event()
            done.record(lane["stream"])
            main.wait_event(done)
            self.emb_g.add_(lane["emb_g"])
            self.mlp_g.add_(lane["mlp_g"])
            self.loss.add_(lane["loss"])
            lane["emb_g"].zero_()
            lane["mlp_g"].zero_()
        fused._bump(self.device)
        return self.acc[:n]

    def scatter_overflow(self, n_rays):
        """Diagnostic: contributions of the last backward that fell back to atomics (synchronises)."""
        cfg = self._cfg()
        n_points = n_rays * self.n_samples
        ws = fused.workspace(cfg, n_points, self.device)
        out = ctypes.c_uint32(0)
        _abi.check(_abi.lib().naf_scatter_overflow_count(ctypes.byref(cfg), n_points, _abi.ptr(ws), ctypes.byref(out)),
                   "scatter_overflow_count")
        return int(out.value)

    def scatter_overflow_levels(self, n_rays):
        """Diagnostic: the same per level (list of num_levels counts; synchronises)."""
        cfg = self._cfg()
        n_points = n_rays * self.n_samples
        ws = fused.workspace(cfg, n_points, self.device)
        out = (ctypes.c_uint32 * 32)()
        _abi.check(_abi.lib().naf_scatter_overflow_levels(ctypes.byref(cfg), n_points, _abi.ptr(ws), ctypes.byref(out)),
                   "scatter_overflow_levels")
        return [int(v) for v in out][:self.net.encoder.num_levels]

    def all_reduce_grads(self):
        """Single-buffer form (one all-reduce of table + MLP gradients + loss); the training step uses the bucketed,
        overlapped form of parallel.py.  Kept for callers that fill the gradient buffers themselves."""
        naf_dist.all_reduce_sum_([self.grad_flat], self.process_group)       # table + MLP gradients + loss (sum over ranks)

    def _adam(self, param, m, v, g, lp, lp_code, what, grad_scale=1.0):
        b1, b2 = self.betas
        _abi.check(_abi.lib().naf_adam_step(_abi.ptr(param), _abi.ptr(m), _abi.ptr(v), _abi.ptr(g), _abi.ptr(lp), lp_code,
                                            param.numel(), self.lr, b1, b2, self.eps, self.step_count, grad_scale, 1,
                                            _abi.stream_ptr()), what)

    def _adam_rows(self, a, e, what="adam_step(table rows)"):
        """Adam on the elements [a, e) of the flat table (master, moments, gradient, 16-bit shadow), gradient cleared: a ragged head
        of up to three elements one by one, the rest in 16-byte groups."""
        emb, m, v, g = (t.view(-1) for t in (self.emb, self.emb_m, self.emb_v, self.emb_g))
        lp = None if self.emb_lp is None else self.emb_lp.view(-1)
        head = min(e, a + (-a) % 4)
        for lo, hi in ((a, head), (head, e)):
            if hi > lo:
                self._adam(emb[lo:hi], m[lo:hi], v[lo:hi], g[lo:hi], None if lp is None else lp[lo:hi], self._lp_code, what)

    def _table_adam(self):
        """struct naf_table_adam for a call that applies the table's Adam update itself, at step `step_count`."""
        b1, b2 = self.betas
        st = _abi.TableAdam()
        st.param, st.exp_avg, st.exp_avg_sq = self.emb.data_ptr(), self.emb_m.data_ptr(), self.emb_v.data_ptr()
        st.param_lp = None if self.emb_lp is None else self.emb_lp.data_ptr()
        st.lp_dtype = self._lp_code
        st.n, st.lr, st.beta1, st.beta2, st.eps, st.step, st.grad_scale = self.emb.numel(), self.lr, b1, b2, self.eps, self.step_count, 1.0
        return st

    def optimizer_step(self, grad_scale=1.0):
        self.step_count += 1
        self._adam(self.emb, self.emb_m, self.emb_v, self.emb_g, self.emb_lp, self._lp_code, "adam_step(table)", grad_scale)
        self._adam(self.mlp, self.mlp_m, self.mlp_v, self.mlp_g, None, 0, "adam_step(mlp)", grad_scale)

    def gather_state(self):
        """Collective, before an evaluation or a checkpoint (trainer.py:113-126): sharded and level-parallel training keep the fp32
        master and the Adam moments of a slice current on its owner only; afterwards every rank holds them all.  Else a no-op."""
        if self._route is not None:
            self._route.gather_state()

    def comm_timing(self, enable=True):
        """Switch on event timing of the exchange (bench.py); `comm_report()` then returns per-step averages."""
        if self._route is not None:
            self._route.timing(enable)

    def comm_report(self):
        """Per-step averages of the timed exchange (parallel.*.report); None without timed steps.  Synchronises."""
        return None if self._route is None else self._route.report()

    def sample_depths(self, rays, t_rand=None, ray_base=0):
        """The sample depths z [n, S] the NEXT train_step / backward on these rays will use (explicit jitter, or the counter-based
        generator keyed by this step's seed and the global ray index): what `raw_noise_std` needs to form its term."""
        cfg = self._cfg(ray_base)
        n = rays.shape[0]
        z = torch.empty(n, self.n_samples, device=self.device)
        _abi.check(_abi.lib().naf_sample_rays(_abi.ptr(rays), _abi.ptr(t_rand), _abi.ptr(z), None, n, self.n_samples, int(self.perturb),
                                              float(self.net.bound), cfg.seed, int(ray_base), _abi.stream_ptr()), "sample_rays")
        return z

    def train_step(self, rays, target, weight, t_rand=None, ray_base=0, raw_noise_std=0.0, noise=None, rays_all=None, global_ray_base=None,
                   next_draw=None):
        """One optimisation step on `rays` [n,8]; loss = sum_r weight[r] (acc[r]-target[r])^2.  Returns the loss tensor
        (device, no sync).  `raw_noise_std` > 0 (render.py:196-199): the per-sample noise on sigma adds sum_s noise_s * dist_s to a
        ray's line integral and nothing else (render.noise_line_integral), so the step runs on target - that term; `noise`: explicit
        N(0, 1) draws [n, S] instead of torch.randn.  `rays_all` / `global_ray_base`: level-parallel steps only
        (parallel.LevelParallelStep.train_step).  `next_draw` (`RayGenerator.plan_draw`): the pixel draw of the NEXT step, carried
        along by this one (naf_render_train_adam_draw: spare workgroups of the scatter's first launch on the fused single-GPU path, a
        launch of its own behind the step otherwise)."""
        n = rays.shape[0]
        if float(raw_noise_std) > 0.0 and n > 0:
            from .render import noise_line_integral
            target = target - noise_line_integral(rays, self.sample_depths(rays, t_rand, ray_base), raw_noise_std, noise)
        if self._route is not None:
            self._route.train_step(rays, target, weight, t_rand, ray_base, rays_all, global_ray_base)
        elif self.fuse_table_adam and (self.n_streams == 1 or n <= self.chunk_rays) and n > 0:
            self._train_step_fused_adam(rays, target, weight, t_rand, ray_base, next_draw)
            next_draw = None
        else:
            self.backward(rays, target, weight, t_rand, ray_base)
            self.optimizer_step()
        if next_draw is not None:
            next_draw.launch()                                 # every other route: the draw as a launch of its own behind the step
        self.rays_seen += n
        return self.loss

    def _train_step_fused_adam(self, rays, target, weight, t_rand, ray_base, next_draw=None):
        """backward() + optimizer_step() in ONE library call: naf_render_train_adam -- the gradient reducer finishes every table
        row with its Adam update, the slab reduction of the MLP gradient does the same for the 4 225 MLP parameters."""
        n = rays.shape[0]
        self._grow_acc(n)
        cfg = self._cfg(ray_base)                              # the jitter seed of step k, as in backward()  (the call overwrites self.loss)
        self.step_count += 1                                   # ... and the Adam step count k + 1, as in optimizer_step()
        ws = fused.workspace(cfg, n * self.n_samples, self.device)
        st = self._table_adam()
        st.mlp_param, st.mlp_exp_avg, st.mlp_exp_avg_sq = self.mlp.data_ptr(), self.mlp_m.data_ptr(), self.mlp_v.data_ptr()
        args = (_abi.ptr(rays), _abi.ptr(t_rand), _abi.ptr(target), _abi.ptr(weight), _abi.ptr(self.table), _abi.ptr(self.offsets),
                _abi.ptr(self.mlp), _abi.ptr(self.acc), _abi.ptr(self.emb_g), _abi.ptr(self.mlp_g), _abi.ptr(self.loss), n,
                ctypes.byref(cfg), _abi.ptr(ws), ctypes.byref(st))
        if next_draw is None:
            _abi.check(_abi.lib().naf_render_train_adam(*args, _abi.stream_ptr()), "render_train_adam")
        else:
            _abi.check(_abi.lib().naf_render_train_adam_draw(*args, ctypes.byref(next_draw), _abi.stream_ptr()), "render_train_adam_draw")
        fused._bump(self.device)                               # (the MLP's update rode on the slab reduction of that call)

    # ---- optimiser state in torch.optim.Adam's layout (checkpoint compatibility, trainer.py:118-126) ---------
    def optimizer_state_dict(self):
        params = [self.net.encoder.embeddings] + [p for lyr in self.net.layers for p in (lyr.weight, lyr.bias)]
        state = {0: {"step": torch.tensor(float(self.step_count)), "exp_avg": self.emb_m.clone(), "exp_avg_sq": self.emb_v.clone()}}
        off = 0
        for i, p in enumerate(params[1:], start=1):
            n = p.numel()
            state[i] = {"step": torch.tensor(float(self.step_count)), "exp_avg": self.mlp_m[off:off + n].view(p.shape).clone(),
                        "exp_avg_sq": self.mlp_v[off:off + n].view(p.shape).clone()}
            off += n
        group = {"lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": 0, "amsgrad": False,
                 "params": list(range(len(params)))}
        return {"state": state, "param_groups": [group]}

    def load_optimizer_state_dict(self, sd):
        st = sd["state"]
        if len(st) == 0:
            return
        self.step_count = int(float(st[0]["step"]))
        self.emb_m.copy_(st[0]["exp_avg"].to(self.device))
        self.emb_v.copy_(st[0]["exp_avg_sq"].to(self.device))
        off = 0
        for i in range(1, len(st)):
            n = st[i]["exp_avg"].numel()
            self.mlp_m[off:off + n].copy_(st[i]["exp_avg"].reshape(-1).to(self.device))
            self.mlp_v[off:off + n].copy_(st[i]["exp_avg_sq"].reshape(-1).to(self.device))
            off += n
        self.lr = float(sd["param_groups"][0]["lr"])

    def sync_from_module(self):
        """Call after net.load_state_dict(): refresh the low-precision shadow table."""
        if self.emb_lp is not None:
            self.emb_lp.copy_(self.emb)
