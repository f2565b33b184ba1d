"""Data-parallel training step on the real engine: two processes (gloo transport, both on the one GPU of the test
box) shard a ray batch, all-reduce the gradients and must end with the parameters of a single process that trained on
the whole batch.  On a multi-GPU node the same code runs with backend "nccl" (RCCL), one process per GPU."""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from _naf_helpers import collect

pytestmark = pytest.mark.gpu


def _make(seed=0):
    from neuralvolumetricreconstructionformedicalimages_amd.encoder import HashEncoder
    from neuralvolumetricreconstructionformedicalimages_amd.network import DensityNetwork
    torch.manual_seed(seed)
    enc = HashEncoder(3, 16, 2, 16, 14)
    enc.embeddings.data.uniform_(-0.1, 0.1)
    net = DensityNetwork(enc, bound=0.3, num_layers=4, hidden_dim=32, skips=[2], out_dim=1, last_activation="sigmoid")
    return net.cuda()


def _batch(n=256, S=64):
    g = torch.Generator().manual_seed(11)
    ang = torch.rand(n, generator=g) * 6.283
    o = torch.stack([torch.cos(ang), torch.sin(ang), torch.zeros(n)], -1)
    d = (torch.rand(n, 3, generator=g) - 0.5) * 0.4 - o
    rays = torch.cat([o, d, torch.full((n, 1), 0.6), torch.full((n, 1), 1.4)], -1)
    return rays, torch.rand(n, S, generator=g), torch.rand(n, generator=g) * 0.3, torch.rand(n, generator=g) > 0.2


_TABLES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def _worker(rank, world, port, out, dp_mode, table, backend="gloo", jitter="explicit"):
    """backend "gloo": every rank on GPU 0 (the one-GPU test box); "nccl": RCCL, rank r on GPU r (a multi-GPU node)."""
    local = rank if backend == "nccl" else 0
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(local),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as td
    from neuralvolumetricreconstructionformedicalimages_amd import dist
    from neuralvolumetricreconstructionformedicalimages_amd.engine import NAFEngine
    torch.cuda.set_device(local)
    if backend == "nccl":
        td.init_process_group("nccl", device_id=torch.device("cuda", local))
    else:
        td.init_process_group("gloo")
    group = td.group.WORLD
    net = _make(seed=0 if rank == 0 else 99)                      # rank 1 starts different until the broadcast
    S = 64
    engine = NAFEngine(net, S, perturb=True, lr=1e-2, process_group=group, dp_mode=dp_mode, table_dtype=_TABLES[table])
    engine.broadcast_parameters()
    rays, t_rand, target, mask = _batch(S=S)
    b, e = dist.shard_range(rays.shape[0], rank, world)
    for _ in range(3):
        w = dist.global_mean_weights(mask[b:e].cuda(), group)
        if jitter == "explicit":
            engine.train_step(rays[b:e].cuda(), target[b:e].cuda(), w, t_rand=t_rand[b:e].cuda().contiguous())
        else:                                                     # counter-based jitter keyed by the global ray index
            engine.train_step(rays[b:e].cuda(), target[b:e].cuda(), w, ray_base=b)
    if dp_mode == "levels":
        engine.gather_state()                                     # level-parallel ranks read only the levels they own between steps
    read = engine.table.float().cpu().numpy()                     # what the next forward would gather from (all-gathered)
    engine.gather_state()                                         # collective: complete fp32 master + moments on every rank
    torch.cuda.synchronize()
    out.put((rank, engine.emb.cpu().numpy(), engine.mlp.cpu().numpy(), float(engine.loss.item()), read, engine.emb_m.cpu().numpy()))
    td.barrier()
    td.destroy_process_group()


@pytest.mark.parametrize("dp_mode,table,jitter", [("sharded", "fp32", "explicit"), ("sharded", "bf16", "explicit"), ("allreduce", "fp32", "explicit"),
                                                  ("allreduce", "bf16", "explicit"), ("levels", "fp32", "explicit"), ("levels", "bf16", "counter"),
                                                  ("sharded", "bf16", "counter")])
def test_two_rank_training_equals_single_process(dp_mode, table, jitter):
    """Two ranks (gloo, sharing the test box's GPU) against one process on the concatenated batch, for the three forms of the
    exchange: all-reduce + replicated Adam, reduce-scatter -> Adam on the rank's table slice -> all-gather (sharded), and
    level-parallel (each rank owns half the levels; features and their gradients cross in two all-to-alls)."""
    from neuralvolumetricreconstructionformedicalimages_amd import dist
    from neuralvolumetricreconstructionformedicalimages_amd.engine import NAFEngine
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29600 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, dp_mode, table, "gloo", jitter)) for r in range(2)]
    for p in procs:
        p.start()
    results = sorted(collect(procs, q, len(procs)), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0

    net = _make(seed=0)
    S = 64
    engine = NAFEngine(net, S, perturb=True, lr=1e-2, table_dtype=_TABLES[table])
    rays, t_rand, target, mask = _batch(S=S)
    for _ in range(3):
        w = dist.global_mean_weights(mask.cuda(), None)
        engine.train_step(rays.cuda(), target.cuda(), w, t_rand=t_rand.cuda() if jitter == "explicit" else None)
    emb, mlp, loss = engine.emb.cpu().numpy(), engine.mlp.cpu().numpy(), float(engine.loss.item())
    for k in (1, 2, 4, 5):                                        # replicas agree: master, MLP, the table they read, moments
        assert np.array_equal(results[0][k], results[1][k]), k
    # the table the kernels read is the (rounded) master everywhere, also for the slices another rank stepped
    assert np.array_equal(results[0][4], torch.from_numpy(results[0][1]).to(_TABLES[table]).float().numpy())
    # Adam steps of +-lr amplify rounding of near-zero gradients, hence the absolute tolerance of a fraction of lr
    np.testing.assert_allclose(results[0][2], mlp, rtol=0, atol=2e-4)
    assert np.mean(np.abs(results[0][1] - emb) > 2e-3) < 1e-3
    np.testing.assert_allclose(results[0][3], loss, rtol=1e-3)
    assert np.mean(np.abs(results[0][5] - engine.emb_m.cpu().numpy()) > 1e-5 * max(1e-12, float(np.abs(results[0][5]).max())) + 1e-9) < 1e-2


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs (RCCL refuses two ranks on one device); the one-GPU "
                                                            "test box runs the gloo variant above")
@pytest.mark.parametrize("dp_mode", ["sharded", "allreduce", "levels"])
def test_two_gpu_rccl_training_equals_single_process(dp_mode):
    """The same comparison over RCCL with one rank per GPU -- the transport the data-parallel step is written for (bucket events
    recorded by the library, collectives on a side stream, per-shard Adam).  Skipped where only one GPU is visible."""
    from neuralvolumetricreconstructionformedicalimages_amd import dist
    from neuralvolumetricreconstructionformedicalimages_amd.engine import NAFEngine
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29700 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, dp_mode, "bf16", "nccl")) for r in range(2)]
    for p in procs:
        p.start()
    results = sorted(collect(procs, q, len(procs)), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    torch.cuda.set_device(0)
    engine = NAFEngine(_make(seed=0), 64, perturb=True, lr=1e-2, table_dtype=torch.bfloat16)
    rays, t_rand, target, mask = _batch(S=64)
    for _ in range(3):
        engine.train_step(rays.cuda(), target.cuda(), dist.global_mean_weights(mask.cuda(), None), t_rand=t_rand.cuda())
    for k in (1, 2, 4, 5):
        assert np.array_equal(results[0][k], results[1][k]), k
    np.testing.assert_allclose(results[0][2], engine.mlp.cpu().numpy(), rtol=0, atol=2e-4)
    assert np.mean(np.abs(results[0][1] - engine.emb.cpu().numpy()) > 2e-3) < 1e-3
    np.testing.assert_allclose(results[0][3], float(engine.loss.item()), rtol=1e-3)


def _empty_shard_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import torch.distributed as td
    from neuralvolumetricreconstructionformedicalimages_amd import dist
    from neuralvolumetricreconstructionformedicalimages_amd.engine import NAFEngine
    td.init_process_group("gloo")
    group = td.group.WORLD
    S = 64
    engine = NAFEngine(_make(seed=0), S, perturb=True, lr=1e-2, process_group=group)
    rays, t_rand, target, mask = _batch(n=3, S=S)
    mask[:] = True
    b, e = (0, 3) if rank == 0 else (3, 3)                        # rank 1 holds NO rays of this step
    for _ in range(2):
        w = dist.global_mean_weights(mask[b:e].cuda(), group)
        engine.train_step(rays[b:e].cuda(), target[b:e].cuda(), w, t_rand=t_rand[b:e].cuda().contiguous())
    torch.cuda.synchronize()
    out.put((rank, engine.emb.cpu().numpy(), engine.mlp.cpu().numpy()))
    td.barrier()
    td.destroy_process_group()


def test_a_rank_without_rays_still_takes_part_in_the_exchange():
    """Three rays on two ranks with rank 1 holding none of them: its (empty) step still records the bucket events, joins every
    all-reduce and applies the summed gradient, so both replicas end with the parameters of the single-process step."""
    from neuralvolumetricreconstructionformedicalimages_amd import dist
    from neuralvolumetricreconstructionformedicalimages_amd.engine import NAFEngine
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 27600 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_empty_shard_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = sorted(collect(procs, q, len(procs)), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    S = 64
    engine = NAFEngine(_make(seed=0), S, perturb=True, lr=1e-2)
    rays, t_rand, target, mask = _batch(n=3, S=S)
    for _ in range(2):
        engine.train_step(rays.cuda(), target.cuda(), torch.full((3,), 1.0 / 3, device="cuda"), t_rand=t_rand.cuda())
    assert np.array_equal(results[0][1], results[1][1]) and np.array_equal(results[0][2], results[1][2])
    np.testing.assert_allclose(results[0][2], engine.mlp.cpu().numpy(), rtol=0, atol=2e-4)
    assert np.mean(np.abs(results[0][1] - engine.emb.cpu().numpy()) > 2e-3) < 1e-3


def _rccl_worker(port, out):
    """World size 1 over the REAL backend ("nccl" = RCCL): the one-GPU test box cannot host two RCCL ranks, but a
    single-rank group drives exactly the code the 8-GPU run uses -- bucket events recorded by the library, the side
    stream waiting on them, ProcessGroupNCCL collectives on slices of the flat buffer, per-bucket Adam."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    import torch.distributed as td
    from neuralvolumetricreconstructionformedicalimages_amd import dist
    from neuralvolumetricreconstructionformedicalimages_amd.engine import NAFEngine
    rank, world, _, group = 0, 1, 0, None
    td.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    group = td.group.WORLD
    res = {}
    for tag, pg, buckets, mode in (("single", None, None, "allreduce"), ("dp", group, None, "allreduce"),
                                   ("dp3", group, [(11, 16), (3, 11), (0, 3)], "allreduce"), ("sharded", group, None, "sharded"),
                                   ("sharded3", group, [(11, 16), (3, 11), (0, 3)], "sharded")):
        net = _make(seed=0)
        S = 64
        engine = NAFEngine(net, S, perturb=True, lr=1e-2, process_group=pg, bucket_levels=buckets, dp_mode=mode)
        engine.broadcast_parameters()
        engine.comm_timing(True)
        rays, t_rand, target, mask = _batch(S=S)
        for _ in range(3):
            w = dist.global_mean_weights(mask.cuda(), pg)
            engine.train_step(rays.cuda(), target.cuda(), w, t_rand=t_rand.cuda())
        torch.cuda.synchronize()
        rep = engine.comm_report()
        res[tag] = (engine.emb.cpu().numpy(), engine.mlp.cpu().numpy(), float(engine.loss.item()), rep)
    out.put(res)
    td.destroy_process_group()


def test_bucketed_rccl_path_with_one_rank_equals_plain_step():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29700 + (os.getpid() % 2000)
    p = ctx.Process(target=_rccl_worker, args=(port, q))
    p.start()
    res = collect([p], q, 1)[0]
    p.join(timeout=120)
    assert p.exitcode == 0
    emb, mlp, loss, rep = res["single"]
    assert rep is None
    for tag in ("dp", "dp3", "sharded", "sharded3"):              # ProcessGroupNCCL all-reduce / reduce-scatter / all-gather on buffer slices
        e, m, l, r = res[tag]
        # same records, same integer row sums; only the rare LDS-overflow atomics may reorder
        np.testing.assert_allclose(m, mlp, rtol=0, atol=1e-6)
        assert np.mean(np.abs(e - emb) > 1e-6) < 1e-4
        np.testing.assert_allclose(l, loss, rtol=1e-6)
        assert r["allreduce_ms_per_step"] >= 0.0 and r["tail_ms_per_step"] > 0.0


@pytest.mark.parametrize("rays,dp_mode,direct", [(1024, "auto", True), (1024, "sharded", True), (8192, "sharded", False)])
def test_bench_two_rank_launch_rehearsal(rays, dp_mode, direct):
    """`bench.py --gpus 2` as the driver may launch it -- bare (`python bench.py --gpus 2`: bench.py starts torch.distributed.run
    itself, as a child process) or already under torch.distributed.run -- except that the two ranks share the one GPU of the test
    box and talk through gloo (NAF_BENCH_BACKEND / NAF_BENCH_SHARE_GPU rehearsal hooks): one JSON line from rank 0 with the
    whole-job rate, the MAX-over-ranks time and the all-reduce probe (exchange times come from the profiled pass: --full)."""
    import json
    import socket
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, NAF_BENCH_BACKEND="gloo", NAF_BENCH_SHARE_GPU="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    tail = [os.path.join(repo, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--rays", str(rays), "--full"]
    if dp_mode != "sharded":                                          # sharded is the default: the driver's command carries no such flag
        tail += ["--dp-mode", dp_mode]
    if direct:
        cmd = [sys.executable, *tail]
    else:
        with socket.socket() as sock:
            sock.bind(("127.0.0.1", 0))
            port = sock.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
               "--master-port", str(port), *tail]
    res = subprocess.run(cmd, cwd=repo, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["scaling"] == "weak"
    assert out["value"] > 0 and abs(out["value"] - 2 * rays * 2 / (out["ms_per_step"] * 2e-3)) < 1e-6 * out["value"]
    assert out["allreduce_ms_per_step"] is not None and out["allreduce_exposed_ms_per_step"] is not None and out["rays_per_s_per_gpu"] > 0
    if dp_mode == "auto":
        # the reference's step: fewer bytes cross the links level-parallel (dist.pick_dp_mode): 2 x 1024 x 192 x 32 x 2 B x 1/2 + MLP
        assert out["config"]["parallelism"] == "lp2" and out["grad_exchange"].startswith("level-parallel")
        assert 12_500_000 < out["allreduce_bytes"] < 12_700_000 and set(out["level_parallel_phases_ms"]) >= {"encode_ms", "features_all_to_all_ms"}
    else:
        assert out["config"]["parallelism"] == "dp2" and out["grad_exchange"].startswith("reduce-scatter")
        assert out["allreduce_bytes"] > 57_000_000
        if rays == 8192:                                              # 8 192 x 192 samples are above dist.SINGLE_BUCKET_BELOW_POINTS
            assert out["allreduce_buckets"] == [[8, 16], [0, 8]]
    assert "cpu_baseline" not in out and "full_schedule" in out and out["full_schedule"] is None      # rank 0 at N = 1 only


@pytest.mark.parametrize("table_dtype,dp_mode", [("float32", "sharded"), ("bfloat16", "sharded"), ("bfloat16", "levels")])
def test_train_py_under_torchrun_equals_the_single_process_run(tmp_path, table_dtype, dp_mode):
    """`python -m torch.distributed.run --nproc-per-node 2 train.py --config ...` (the documented data-parallel launch;
    here the two ranks share the one GPU of the test box and talk through gloo: NAF_DIST_BACKEND / NAF_DIST_SHARE_GPU)
    trains to the same parameters as `python train.py --config ...` on the same seeded pixel draws: the ranks take slices of
    one draw, the loss is the global masked mean, rank 0 evaluates and writes the checkpoint."""
    import pickle
    import socket
    import subprocess
    import sys
    import yaml
    from neuralvolumetricreconstructionformedicalimages_amd.dataset import synthetic_scan
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    data = synthetic_scan(n_voxel=16, n_train=4, n_val=2, device="cuda", seed=0)
    with open(tmp_path / "scan.pickle", "wb") as f:
        pickle.dump(data, f, pickle.HIGHEST_PROTOCOL)

    def config(name):
        cfg = {
            "exp": {"expname": name, "expdir": str(tmp_path), "datadir": str(tmp_path / "scan.pickle")},
            "network": {"net_type": "mlp", "num_layers": 4, "hidden_dim": 32, "skips": [2], "out_dim": 1,
                        "last_activation": "sigmoid", "bound": 0.3},
            "encoder": {"encoding": "hashgrid", "input_dim": 3, "num_levels": 16, "level_dim": 2, "base_resolution": 16,
                        "log2_hashmap_size": 12},
            "render": {"n_samples": 32, "n_fine": 0, "perturb": True, "raw_noise_std": 0.0, "netchunk": 4096},
            "train": {"epoch": 2, "n_batch": 1, "n_rays": 256, "lrate": 5e-3, "lrate_gamma": 0.5, "lrate_step": 1, "resume": False},
            "log": {"i_eval": 2, "i_save": 2},
            "backend": {"engine": "fused", "table_dtype": table_dtype, "loss": "global_mean", "seed": 3, "dp_mode": dp_mode},
        }
        path = tmp_path / f"{name}.yaml"
        path.write_text(yaml.safe_dump(cfg))
        return str(path)

    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ, NAF_DIST_BACKEND="gloo", NAF_DIST_SHARE_GPU="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    dp = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                         "127.0.0.1", "--master-port", str(port), os.path.join(repo, "train.py"), "--config", config("dp")],
                        cwd=repo, env=env, capture_output=True, text=True, timeout=600)
    assert dp.returncode == 0, dp.stderr[-3000:]
    one = subprocess.run([sys.executable, os.path.join(repo, "train.py"), "--config", config("single")],
                         cwd=repo, env=env, capture_output=True, text=True, timeout=600)
    assert one.returncode == 0, one.stderr[-3000:]
    a = torch.load(tmp_path / "dp" / "ckpt.tar", weights_only=False)
    b = torch.load(tmp_path / "single" / "ckpt.tar", weights_only=False)
    assert a["epoch"] == b["epoch"] == 2
    for key in b["network"]:
        x, y = a["network"][key].float().cpu(), b["network"][key].float().cpu()
        if table_dtype == "float32":
            assert float((x - y).abs().max()) <= 2e-5 * max(float(y.abs().max()), 1e-3), key
        else:      # bf16 records: sums differ in their last bits, Adam turns a near-zero gradient into a step of +-lr on a few rows
            assert float(((x - y).abs() > 1e-2 * max(float(y.abs().max()), 1e-3)).float().mean()) < 1e-2, key
    # the checkpoint holds the COMPLETE optimiser state and fp32 master table although every rank steps only its shard / its levels
    # (Trainer gathers them before it evaluates and before it saves)
    ma, mb = a["optimizer"]["state"][0]["exp_avg"].float().cpu(), b["optimizer"]["state"][0]["exp_avg"].float().cpu()
    tol = (1e-4 if table_dtype == "float32" else 3e-2) * float(mb.abs().max())
    assert float(((ma - mb).abs() > tol).float().mean()) < 1e-2
    assert os.path.exists(tmp_path / "dp" / "eval" / "epoch_00002" / "stats.txt")
    assert dp.stdout.count("[SAVE]") == 1                                  # rank 0 only
