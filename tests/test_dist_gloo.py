"""world_size-2 data-parallel logic on CPU (gloo): ray sharding + global-mean weights + gradient all-reduce give the
single-process gradient of the concatenated batch.  The HIP engine uses exactly these helpers
(engine.NAFEngine.all_reduce_grads / dist.global_mean_weights) with backend "nccl" (RCCL) on the GPUs."""
import os

import numpy as np
import torch
import torch.distributed as td
import torch.multiprocessing as mp

from _naf_helpers import collect

from neuralvolumetricreconstructionformedicalimages_amd import dist


def _model_grads(params, x, y, w):
    """A small stand-in 'renderer' (the real one needs a GPU): acc = sigmoid(x @ W1) @ w2."""
    W1, w2 = (p.clone().requires_grad_(True) for p in params)
    acc = torch.sigmoid(x @ W1) @ w2
    loss = (w * (acc - y) ** 2).sum()
    loss.backward()
    return [W1.grad, w2.grad], loss.detach()


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    r, w, _, group = dist.init_from_env(device_type="cpu")
    assert (r, w) == (rank, world)
    g = torch.Generator().manual_seed(0)
    n = 101
    x, y = torch.randn(n, 6, generator=g), torch.randn(n, generator=g)
    mask = torch.rand(n, generator=g) > 0.25
    params = [torch.randn(6, 5, generator=g), torch.randn(5, generator=g)]
    if rank != 0:                                   # ranks start from different weights until the broadcast
        params = [p + 1.0 for p in params]
    dist.broadcast_parameters(params, group)
    b, e = dist.shard_range(n, rank, world)
    weights = dist.global_mean_weights(mask[b:e], group)
    grads, loss = _model_grads(params, x[b:e], y[b:e], weights)
    loss = loss.reshape(1)
    dist.all_reduce_sum_(grads + [loss], group)
    q.put((rank, [t.numpy() for t in grads], float(loss)))
    td.barrier()
    td.destroy_process_group()


def test_dp_gradients_equal_single_process():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = collect(procs, q, len(procs), timeout=120)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    g = torch.Generator().manual_seed(0)
    n = 101
    x, y = torch.randn(n, 6, generator=g), torch.randn(n, generator=g)
    mask = torch.rand(n, generator=g) > 0.25
    params = [torch.randn(6, 5, generator=g), torch.randn(5, generator=g)]
    ref_grads, ref_loss = _model_grads(params, x, y, dist.global_mean_weights(mask, None))
    for rank, grads, loss in results:
        np.testing.assert_allclose(loss, float(ref_loss), rtol=1e-5)
        for a, b in zip(grads, ref_grads):
            np.testing.assert_allclose(a, b.numpy(), rtol=1e-4, atol=1e-6)


# ---- bucketed exchange: the collectives parallel.AllReduceExchange issues per level bucket ------------------------------
def _bucket_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    _, _, _, group = dist.init_from_env(device_type="cpu")
    from neuralvolumetricreconstructionformedicalimages_amd.encoder import level_offsets
    offs = level_offsets(3, 16, 16, 14)
    C = 2
    n_emb = int(offs[-1]) * C
    o_mlp = (n_emb + 63) // 64 * 64
    total = o_mlp + (4225 + 63) // 64 * 64 + 64                     # table | MLP | loss, as engine.NAFEngine lays it out
    g = torch.Generator().manual_seed(100 + rank)
    flat = torch.randn(total, generator=g)
    whole = flat.clone()
    td.all_reduce(whole, group=group)                               # the single-buffer exchange
    buckets = dist.default_bucket_levels(16)
    slices = dist.grad_bucket_slices(offs, C, buckets)
    dist.all_reduce_buckets_(flat, [(o_mlp, total)] + slices, group)
    q.put((rank, bool(torch.equal(flat[:n_emb], whole[:n_emb])), bool(torch.equal(flat[o_mlp:], whole[o_mlp:])), slices, buckets))
    td.barrier()
    td.destroy_process_group()


def test_bucketed_exchange_equals_single_all_reduce():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_bucket_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = collect(procs, q, len(procs), timeout=120)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, table_ok, mlp_ok, slices, buckets in results:
        assert table_ok and mlp_ok
        assert buckets == [(8, 16), (0, 8)]                          # fine half first (its exchange hides behind the coarse half's
        #                                                              reduction); halves keep every reducer launch unsplit = deterministic
        assert slices[1][0] == 0 and slices[1][1] == slices[0][0]    # the slices tile the table exactly once
    with np.testing.assert_raises(ValueError):
        dist.grad_bucket_slices([0, 10, 20, 30], 2, [(0, 2), (1, 3)])           # overlap
    with np.testing.assert_raises(ValueError):
        dist.grad_bucket_slices([0, 10, 20, 30], 2, [(0, 2)])                   # level 2 missing
    assert dist.grad_bucket_slices([0, 10, 20, 30], 2, [(2, 3), (0, 2)]) == [(40, 60), (0, 40)]


# ---- sharded optimiser: reduce-scatter -> Adam on the rank's slice -> all-gather (parallel.ShardedExchange) --------------------
def _adam_ref(p, m, v, g, step, lr=1e-2, b1=0.9, b2=0.999, eps=1e-8):
    m.mul_(b1).add_(g, alpha=1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    p.addcdiv_(m / (1 - b1 ** step), (v / (1 - b2 ** step)).sqrt() + eps, value=-lr)


def _sharded_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    _, _, _, group = dist.init_from_env(device_type="cpu")
    from neuralvolumetricreconstructionformedicalimages_amd.encoder import level_offsets
    offs = level_offsets(3, 16, 16, 12)
    C = 2
    n_emb = int(offs[-1]) * C
    n_pad = dist.padded_length(n_emb, world)                        # the engine's padding rule: lcm(64, 4 * world)
    slices = dist.grad_bucket_slices(offs, C, [(11, 16), (3, 11), (0, 3)])
    ranges = dist.sharded_exchange_slices(slices, world, n_pad)
    g0 = torch.Generator().manual_seed(7)
    p_ref = torch.randn(n_emb, generator=g0)
    p = torch.zeros(n_pad)
    p[:n_emb] = p_ref
    m, v = torch.zeros(n_emb), torch.zeros(n_emb)
    m_ref, v_ref = torch.zeros(n_emb), torch.zeros(n_emb)
    for step in (1, 2, 3):
        grad = torch.zeros(n_pad)
        grad[:n_emb] = torch.randn(n_emb, generator=torch.Generator().manual_seed(1000 * step + rank))
        whole = grad.clone()
        td.all_reduce(whole, group=group)
        _adam_ref(p_ref, m_ref, v_ref, whole[:n_emb], step)        # the all-reduce form, every rank the whole table
        for a, b in ranges:                                        # the sharded form
            lo, end, hi = dist.shard_bounds(a, b, world, rank, n_emb)
            out = torch.zeros(end - lo)
            td.reduce_scatter_tensor(out, grad[a:b].contiguous(), group=group)
            if hi > lo:
                _adam_ref(p[lo:hi], m[lo:hi], v[lo:hi], out[:hi - lo], step)
            td.all_gather_into_tensor(p[a:b], p[lo:end].clone(), group=group)
    owned = torch.zeros(n_emb, dtype=torch.bool)
    for a, b in ranges:
        lo, _, hi = dist.shard_bounds(a, b, world, rank, n_emb)
        owned[lo:hi] = True
    exact = world == 2                                             # a sum of three addends depends on the order the backend takes them in
    same_p = torch.equal(p[:n_emb], p_ref) if exact else torch.allclose(p[:n_emb], p_ref, rtol=0, atol=2e-4)   # Adam steps of lr = 1e-2
    same_m = torch.equal(m[owned], m_ref[owned]) if exact else torch.allclose(m[owned], m_ref[owned], rtol=1e-5, atol=1e-6)
    q.put((rank, bool(same_p), bool(same_m), float(owned.float().mean()), ranges, n_pad))
    td.barrier()
    td.destroy_process_group()


def _run_sharded(world, port):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_sharded_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = collect(procs, q, len(procs), timeout=120)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return results


def test_sharded_optimizer_exchange_equals_all_reduce_then_adam():
    """reduce-scatter -> per-rank Adam on a 1/N slice -> all-gather leaves every rank with the parameters of all-reduce -> Adam
    on the whole table -- bit for bit with 2 ranks (a sum of two addends has one order), to rounding with 3 (a world size
    that does not divide the buffer's 64-element granule: the padding rule is lcm(64, 4 * world))."""
    for world, port in ((2, 33500 + (os.getpid() % 1000)), (3, 35500 + (os.getpid() % 1000))):
        for rank, params_equal, moments_equal, share, ranges, n_pad in _run_sharded(world, port):
            assert params_equal and moments_equal
            assert abs(share - 1.0 / world) < 0.01                   # every rank steps 1/N of the table
            assert ranges[-1][0] == 0 and max(b for _, b in ranges) == n_pad
            assert all((b - a) % (4 * world) == 0 and a % 4 == 0 for a, b in ranges)


# ---- level-parallel exchange (parallel.LevelParallelStep): the two all-to-alls, on CPU -------------------------------------------
def _levels_worker(rank, world, port, q):
    """A per-level linear 'encoder' stands in for the hash grid: feature(l, point) = table[l] * x(point).  Rank k owns L / world
    levels; the features of its levels for every rank's points go out in one block per destination, the gradients come back the
    same way -- the buffer layouts of naf_levels_encode / naf_levels_field_step / naf_levels_scatter."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    _, _, _, group = dist.init_from_env(device_type="cpu")
    L, run = 8, 5                                   # levels, points x C of one rank
    per = L // world
    g = torch.Generator().manual_seed(3)
    table = torch.randn(L, generator=g)             # every rank knows the whole table here; it READS only the levels it owns
    x_all = torch.randn(world, run, generator=g)    # rank r's points
    head = torch.randn(L, generator=g)              # the 'MLP': acc = sum_l head[l] * feature[l]
    lb = rank * per
    send = torch.stack([torch.stack([table[lb + l] * x_all[r] for l in range(per)]) for r in range(world)])      # [dest][owned level][run]
    feat = torch.empty(L, run)
    td.all_to_all_single(feat.view(-1), send.view(-1), group=group)          # block k = rank k's levels of MY points -> [L][run]
    want = table[:, None] * x_all[rank][None, :]
    assert torch.equal(feat, want)
    dfeat = head[:, None] * torch.ones(L, run) * (rank + 1)                  # d loss / d feature of my points, [L][run]
    recv = torch.empty(world, per * run)
    td.all_to_all_single(recv.view(-1), dfeat.view(-1), group=group)         # block k = rank k's gradients of MY levels
    grad_owned = torch.stack([sum(recv[r].view(per, run)[l] @ x_all[r] for r in range(world)) for l in range(per)])
    q.put((rank, grad_owned.numpy()))
    td.barrier()
    td.destroy_process_group()


def test_level_parallel_exchange_layout_gives_the_single_process_table_gradient():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + ((os.getpid() + 77) % 2000)
    procs = [ctx.Process(target=_levels_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = sorted(collect(procs, q, len(procs), timeout=120), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    L, run = 8, 5
    g = torch.Generator().manual_seed(3)
    table = torch.randn(L, generator=g).requires_grad_(True)
    x_all = torch.randn(world, run, generator=g)
    head = torch.randn(L, generator=g)
    loss = sum((r + 1) * (head[:, None] * (table[:, None] * x_all[r][None, :])).sum() for r in range(world))
    loss.backward()
    got = np.concatenate([r[1] for r in results])
    np.testing.assert_allclose(got, table.grad.numpy(), rtol=1e-5, atol=1e-6)


def test_pick_dp_mode_by_bytes_on_the_links():
    chest = dict(num_levels=16, level_dim=2, table_elements=14262438)
    assert dist.pick_dp_mode(1, points_per_step=1024 * 192, **chest) == "sharded"             # nothing to exchange
    assert dist.pick_dp_mode(8, points_per_step=1024 * 192, **chest) == "levels"              # 25 MB against 85.5 MB
    assert dist.pick_dp_mode(8, points_per_step=3072 * 192, **chest) == "levels"
    assert dist.pick_dp_mode(8, points_per_step=4096 * 192, **chest) == "sharded"             # 100 MB against 85.5 MB
    assert dist.pick_dp_mode(8, points_per_step=65536 * 192, **chest) == "sharded"
    assert dist.pick_dp_mode(3, points_per_step=1024 * 192, **chest) == "sharded"             # 16 levels do not split three ways
    assert dist.pick_dp_mode(8, points_per_step=None, **chest) == "sharded"                   # unknown batch: the safe choice
    assert dist.pick_dp_mode(8, points_per_step=2048 * 192, feature_bytes=4, table_bytes=4, **chest) == "levels"      # fp32: 100 MB against 114 MB
