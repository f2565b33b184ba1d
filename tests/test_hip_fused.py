"""GPU parity of the fused ray-march path (naf_render_forward / _backward / _train, naf_field_forward) against
the CPU oracle and the golden vectors captured from the reference.

Bars (BASELINE.json north_star): projection relative L2 <= 1e-4 in fp32 parity mode; bf16-MFMA mode is checked
against the fp32 result with the looser tolerances written in each test."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _mods():
    from neuralvolumetricreconstructionformedicalimages_amd import _abi, encoder, fused, network
    return _abi, encoder, fused, network


def _rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _build_net(g, prefix="net"):
    _abi, encoder, fused, network = _mods()
    enc = encoder.HashEncoder(**{k: int(g[f"enc/{k}"]) for k in
                                 ("input_dim", "num_levels", "level_dim", "base_resolution", "log2_hashmap_size")})
    enc.embeddings.data.copy_(torch.from_numpy(g["enc/embeddings"]))
    net = network.DensityNetwork(enc, bound=0.3, num_layers=4, hidden_dim=32, skips=[2], out_dim=1, last_activation="sigmoid")
    for i, lyr in enumerate(net.layers):
        lyr.weight.data.copy_(torch.from_numpy(g[f"{prefix}/w{i}"]))
        lyr.bias.data.copy_(torch.from_numpy(g[f"{prefix}/b{i}"]))
    return net.cuda()


# golden encoder has L=8, C=2 (16 features) -> not the fused shape; it exercises the unfused composition instead
def test_unfused_module_path_matches_reference_golden(golden):
    from neuralvolumetricreconstructionformedicalimages_amd import render as R
    g = golden("render")
    net = _build_net(g)
    assert not net.fused_supported()
    rays = torch.from_numpy(g["rays"]).cuda()
    S = g["det/t_rand"].shape[1]
    for tag, perturb in (("det", False), ("jit", True)):
        net.zero_grad()
        ret = R.render(rays, net, None, S, 0, perturb, 4096, 0.0, t_rand=torch.from_numpy(g[f"{tag}/t_rand"]).cuda())
        assert _rel_l2(ret["acc"].detach().cpu().numpy(), g[f"{tag}/acc"]) < 1e-5
        np.testing.assert_allclose(ret["pts"].cpu().numpy(), g[f"{tag}/pts"], rtol=0, atol=1.2e-7)
        loss = ((ret["acc"] - torch.from_numpy(g[f"{tag}/target"]).cuda()) ** 2).mean()
        loss.backward()
        ge = g[f"{tag}/g_embeddings"]
        np.testing.assert_allclose(net.encoder.embeddings.grad.cpu().numpy(), ge, rtol=0, atol=3e-5 * np.abs(ge).max())
        for i, lyr in enumerate(net.layers):
            gw = g[f"{tag}/gw{i}"]
            np.testing.assert_allclose(lyr.weight.grad.cpu().numpy(), gw, rtol=0, atol=3e-5 * max(np.abs(gw).max(), 1e-12))


def _naf_pair(seed=0, log2T=14, scale=0.5, last_activation="sigmoid", L=16, C=2, H=16):
    """Canonical NAF network (L=16,C=2,H=16 -> 32 features) on GPU + the oracle twin on CPU with equal weights."""
    _abi, encoder, fused, network = _mods()
    from oracle.hashgrid_ref import HashEncoderRef
    from oracle.network_ref import DensityNetworkRef
    torch.manual_seed(seed)
    enc = encoder.HashEncoder(3, L, C, H, log2T)
    enc.embeddings.data.uniform_(-scale, scale)
    net = network.DensityNetwork(enc, bound=0.3, num_layers=4, hidden_dim=32, skips=[2], out_dim=1,
                                 last_activation=last_activation)
    ref_enc = HashEncoderRef(3, L, C, H, log2T)
    ref_enc.embeddings.data.copy_(enc.embeddings.data)
    ref = DensityNetworkRef(ref_enc, bound=0.3, num_layers=4, hidden_dim=32, skips=(2,), out_dim=1,
                            last_activation=last_activation)
    for a, b in zip(ref.layers, net.layers):
        a.weight.data.copy_(b.weight.data)
        a.bias.data.copy_(b.bias.data)
    return net.cuda(), ref


def _rays(n, seed=1):
    g = torch.Generator().manual_seed(seed)
    ang = torch.rand(n, generator=g) * 6.283
    o = torch.stack([torch.cos(ang), torch.sin(ang), (torch.rand(n, generator=g) - 0.5) * 0.2], -1)
    tgt = (torch.rand(n, 3, generator=g) - 0.5) * 0.5
    d = tgt - o
    d = d / d.norm(dim=-1, keepdim=True) * (0.8 + 0.4 * torch.rand(n, 1, generator=g))     # un-normalised like cone rays
    return torch.cat([o, d, torch.full((n, 1), 0.6), torch.full((n, 1), 1.4)], -1)


@pytest.mark.parametrize("S,perturb", [(64, False), (192, True), (50, True)])
def test_fused_forward_fp32_vs_oracle(S, perturb):
    from oracle import render_ref as R
    _abi, encoder, fused, network = _mods()
    net, ref = _naf_pair()
    assert net.fused_supported()
    rays = _rays(37)
    t_rand = torch.rand(37, S, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        want = R.render(rays, ref, None, S, 0, perturb, 1 << 20, 0.0, t_rand=t_rand)["acc"].numpy()
        got = fused.fused_render(rays.cuda(), net, S, perturb, t_rand=t_rand.cuda()).cpu().numpy()
    assert _rel_l2(got, want) < 1e-4          # north_star: projection L2 within 1e-4 relative
    np.testing.assert_allclose(got, want, rtol=2e-4, atol=1e-6)


@pytest.mark.parametrize("act", ["sigmoid", "relu", "tanh", "none"])
def test_fused_backward_fp32_vs_oracle(act):
    from oracle import render_ref as R
    _abi, encoder, fused, network = _mods()
    net, ref = _naf_pair(seed=2, last_activation=act)
    S, n = 96, 29
    rays = _rays(n, seed=5)
    t_rand = torch.rand(n, S, generator=torch.Generator().manual_seed(4))
    target = torch.rand(n, generator=torch.Generator().manual_seed(6)) * 0.3
    acc_ref = R.render(rays, ref, None, S, 0, True, 1 << 20, 0.0, t_rand=t_rand)["acc"]
    ((acc_ref - target) ** 2).mean().backward()
    acc = fused.fused_render(rays.cuda(), net, S, True, t_rand=t_rand.cuda())
    ((acc - target.cuda()) ** 2).mean().backward()
    assert _rel_l2(acc.detach().cpu().numpy(), acc_ref.detach().numpy()) < 1e-4
    for a, b in zip(net.layers, ref.layers):
        gw, gb = b.weight.grad.numpy(), b.bias.grad.numpy()
        assert _rel_l2(a.weight.grad.cpu().numpy(), gw) < 2e-4, act
        assert _rel_l2(a.bias.grad.cpu().numpy(), gb) < 2e-4, act
    ge = ref.encoder.embeddings.grad.numpy()
    assert _rel_l2(net.encoder.embeddings.grad.cpu().numpy(), ge) < 2e-4


@pytest.mark.parametrize("L,C", [(8, 4), (4, 8)])
@pytest.mark.parametrize("scatter_mode", [1, 2])
def test_fused_other_level_shapes_fp32_vs_oracle(L, C, scatter_mode):
    """The fused kernels are templated on the channels per level; every L x C = 32 split runs the same MLP.  Forward
    and all gradients against the oracle, with the atomic (1) and the binned (2) table-gradient scatter.
    (C = 1 needs L = 32, whose top levels exceed fp32 coordinate resolution -- the torch oracle's unfused x*scale+0.5
    then picks other cells than the fma of the kernels and of the C oracle; that shape is covered by the
    binned-vs-atomic and the in-bounds tests below.)"""
    from oracle import render_ref as R
    _abi, encoder, fused, network = _mods()
    net, ref = _naf_pair(seed=11, log2T=12, L=L, C=C)
    assert net.fused_supported()
    S, n = 64, 33
    rays = _rays(n, seed=31)
    t_rand = torch.rand(n, S, generator=torch.Generator().manual_seed(8))
    target = torch.rand(n, generator=torch.Generator().manual_seed(9)) * 0.3
    acc_ref = R.render(rays, ref, None, S, 0, True, 1 << 20, 0.0, t_rand=t_rand)["acc"]
    ((acc_ref - target) ** 2).mean().backward()
    with fused.scatter_mode(scatter_mode):
        acc = fused.fused_render(rays.cuda(), net, S, True, t_rand=t_rand.cuda())
        ((acc - target.cuda()) ** 2).mean().backward()
    assert _rel_l2(acc.detach().cpu().numpy(), acc_ref.detach().numpy()) < 1e-4
    for a, b in zip(net.layers, ref.layers):
        assert _rel_l2(a.weight.grad.cpu().numpy(), b.weight.grad.numpy()) < 2e-4
    assert _rel_l2(net.encoder.embeddings.grad.cpu().numpy(), ref.encoder.embeddings.grad.numpy()) < 2e-4


@pytest.mark.parametrize("L,C", [(32, 1), (8, 4), (4, 8)])
def test_fused_other_level_shapes_bf16_binned_equals_atomic(L, C):
    _abi, encoder, fused, network = _mods()
    net, _ = _naf_pair(seed=12, log2T=15, scale=0.1, L=L, C=C, H=1 if L == 32 else 16)
    n, S = 1024, 96
    rays = _rays(n, seed=37).cuda()
    target = torch.rand(n, device="cuda") * 0.3
    grads = {}
    for mode in (1, 2):
        with fused.scatter_mode(mode):
            net.zero_grad()
            acc = fused.fused_render(rays, net, S, True, seed=5, mlp_precision=_abi.BF16)
            ((acc - target) ** 2).mean().backward()
            grads[mode] = net.encoder.embeddings.grad.clone()
    a, b = grads[1].double(), grads[2].double()
    assert float((a - b).norm() / a.norm()) < 3e-3


def test_levels_beyond_uint32_resolution_stay_in_bounds():
    """L=32 at H=16 asks for resolutions up to 2^35: the float -> uint32 conversions saturate (as in the reference's
    CUDA build) and every such level must still index inside its table (mask / modulo path), forward and backward."""
    _abi, encoder, fused, network = _mods()
    torch.manual_seed(0)
    enc = encoder.HashEncoder(3, 32, 1, 16, 12).cuda()
    x = (torch.rand(4096, 3, device="cuda") - 0.5) * 0.59
    x.requires_grad_(False)
    y = enc(x, 0.3)
    assert y.shape == (4096, 32) and bool(torch.isfinite(y).all())
    # up to level 28 (scale 2^32 - 1) positions fit uint32: values come from inside the U(-1e-4, 1e-4) table
    assert float(y[:, :29].detach().abs().max()) <= 1e-4 + 1e-7
    # beyond, the cell index saturates at 2^32 - 1 and the reference's `pos -= (float)pos_grid` (hashencoder.cu:109-110) leaves
    # a huge "fraction": the weights extrapolate (finite garbage, identical in the reference) -- what matters is that every
    # gather and scatter stays inside its level
    y[:, :29].sum().backward(retain_graph=True)
    g = enc.embeddings.grad
    assert bool(torch.isfinite(g).all()) and abs(float(g.sum()) - 4096 * 29) < 1.0     # every corner weight landed in the table
    offs = enc.offsets.tolist()
    assert float(g[offs[29]:].abs().max()) == 0.0                                      # nothing leaked into other levels
    enc.embeddings.grad = None
    y[:, 29:].sum().backward()                                                         # saturated levels: in bounds, no fault
    g = enc.embeddings.grad
    assert bool(torch.isfinite(g).all()) and float(g[:offs[29]].abs().max()) == 0.0


def test_render_train_entry_matches_autograd_path():
    """naf_render_train (forward + weighted MSE + backward in one call) == autograd through fused_render."""
    _abi, encoder, fused, network = _mods()
    net, _ = _naf_pair(seed=3)
    S, n = 192, 64
    rays = _rays(n, seed=7).cuda()
    t_rand = torch.rand(n, S, device="cuda")
    target = torch.rand(n, device="cuda") * 0.3
    mask = (torch.rand(n, device="cuda") > 0.2).float()
    weight = mask / mask.sum()
    acc = fused.fused_render(rays, net, S, True, t_rand=t_rand)
    loss = (weight * (acc - target) ** 2).sum()
    loss.backward()
    cfg = fused.render_cfg(net, S, True)
    ws = fused.workspace(cfg, n * S, rays.device)
    acc2 = torch.empty(n, device="cuda")
    g_emb = torch.zeros_like(net.encoder.embeddings)
    g_mlp = torch.zeros(_abi.MLP_PARAMS, device="cuda")
    loss2 = torch.zeros(1, device="cuda")
    mlp = net.packed_mlp().detach().contiguous()
    _abi.check(_abi.lib().naf_render_train(_abi.ptr(rays), _abi.ptr(t_rand), _abi.ptr(target), _abi.ptr(weight),
                                           _abi.ptr(net.encoder.embeddings.detach()), _abi.ptr(net.encoder.offsets), _abi.ptr(mlp),
                                           _abi.ptr(acc2), _abi.ptr(g_emb), _abi.ptr(g_mlp), _abi.ptr(loss2), n, ctypes.byref(cfg),
                                           _abi.ptr(ws), _abi.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(acc2, acc.detach())
    np.testing.assert_allclose(loss2.item(), loss.item(), rtol=1e-5)
    want = torch.cat([torch.cat([l.weight.grad.reshape(-1), l.bias.grad.reshape(-1)]) for l in net.layers])
    assert torch.equal(g_mlp, want)                  # slab reduction is deterministic
    ge = net.encoder.embeddings.grad
    assert _rel_l2(g_emb.cpu().numpy(), ge.cpu().numpy()) < 1e-5     # fp32 atomics: order differs run to run


def test_fused_bf16_close_to_fp32():
    _abi, encoder, fused, network = _mods()
    net, _ = _naf_pair(seed=4)
    S, n = 192, 128
    rays = _rays(n, seed=9).cuda()
    t_rand = torch.rand(n, S, device="cuda")
    target = torch.rand(n, device="cuda") * 0.3
    out = {}
    for tag, prec in (("f32", _abi.F32), ("bf16", _abi.BF16)):
        net.zero_grad()
        acc = fused.fused_render(rays, net, S, True, t_rand=t_rand, mlp_precision=prec)
        ((acc - target) ** 2).mean().backward()
        out[tag] = (acc.detach().cpu().numpy(), net.encoder.embeddings.grad.cpu().numpy().copy(),
                    [l.weight.grad.cpu().numpy().copy() for l in net.layers])
    assert _rel_l2(out["bf16"][0], out["f32"][0]) < 1e-2          # bf16 operands: ~3 significant digits
    assert _rel_l2(out["bf16"][1], out["f32"][1]) < 5e-2
    for a, b in zip(out["bf16"][2], out["f32"][2]):
        assert _rel_l2(a, b) < 5e-2


@pytest.mark.parametrize("L,C", [(16, 2), (8, 4), (4, 8)])
def test_bf16_mode_matches_a_bf16_rounding_emulation(L, C):
    """bf16 mode is not "approximately fp32", it is exactly: features, weights and hidden activations rounded to bf16
    (round-to-nearest-even) where they enter an MFMA, fp32 accumulation, fp32 output layer.  Emulating those roundings
    on the oracle's fp32 features reproduces the kernel to fp32 summation-order noise -- a 1000x tighter check of the
    bf16 kernels than the comparison with the fp32 mode."""
    _abi, encoder, fused, network = _mods()
    net, ref = _naf_pair(seed=15, log2T=12, L=L, C=C)
    pts = (torch.rand(3000, 3, generator=torch.Generator().manual_seed(4)) - 0.5) * 0.59
    r = lambda t: t.bfloat16().float()                                                  # noqa: E731
    with torch.no_grad():
        x = r(ref.encoder(pts, 0.3))
        W = [r(l.weight) for l in ref.layers[:3]]
        b = [l.bias for l in ref.layers]
        leaky = torch.nn.functional.leaky_relu
        h1 = leaky(x @ W[0].T + b[0], 0.01)
        h2 = leaky(r(h1) @ W[1].T + b[1], 0.01)
        h3 = leaky(torch.cat([x, r(h2)], -1) @ W[2].T + b[2], 0.01)
        want = torch.sigmoid(h3 @ ref.layers[3].weight.T + b[3]).reshape(-1)
        got = fused.field_query(net, pts.cuda(), mlp_precision=_abi.BF16).cpu().reshape(-1)
    assert _rel_l2(got.numpy(), want.numpy()) < 2e-6
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=2e-5, atol=1e-7)


@pytest.mark.parametrize("S", [64, 50, 7, 200])
def test_bf16_mode_backward_matches_a_bf16_rounding_emulation(S):
    """Same idea for the backward pass: every MFMA operand (gradient tiles, activations, transposed weights) rounded to
    bf16, fp32 accumulation, masks and the output layer in fp32.  Checks the MLP weight gradients and, through the
    atomic scatter, the table gradient (feature gradients are stored as bf16)."""
    from oracle import render_ref as R
    from oracle.hashgrid_ref import hash_encode_backward
    _abi, encoder, fused, network = _mods()
    net, ref = _naf_pair(seed=16, log2T=12)
    n = 24                                   # S = 50, 7, 200: the last 16-point tile of a ray is ragged
    rays = _rays(n, seed=47)
    t_rand = torch.rand(n, S, generator=torch.Generator().manual_seed(5))
    target = torch.rand(n, generator=torch.Generator().manual_seed(6)) * 0.3
    # the roundings themselves live in tests/_mlp16_oracle.py (shared with the float64 reference of test_hip_mlp16_reference.py); here
    # in fp32, on the upstream gradient of a mean squared error: weight 1 / n
    import _mlp16_oracle as O
    with torch.no_grad():
        z = R.sample_depths(rays[:, 6:7], rays[:, 7:8], S, True, t_rand)
        pts = R.points_on_rays(rays, z, 0.3).reshape(-1, 3)
        dn = rays[:, 3:6].norm(dim=-1, keepdim=True)
        dist = torch.cat([z[:, 1:] - z[:, :-1], torch.full((n, 1), 1e-10)], -1) * dn
        emu = O.rehearse(ref.encoder(pts, 0.3).reshape(n, S, 32), dist, target, torch.full((n,), 1.0 / n), ref.layers, dtype=torch.float32)
    acc_want, dx = emu["acc"], emu["dx"]
    dW0, dW1, dW2, dw3 = emu["blocks"][0], emu["blocks"][2], emu["blocks"][4], emu["blocks"][6]
    r = lambda t: t.bfloat16().float()                                                  # noqa: E731
    with fused.scatter_mode(1):          # the mode travels in the cfg captured by the forward call
        acc = fused.fused_render(rays.cuda(), net, S, True, t_rand=t_rand.cuda(), mlp_precision=_abi.BF16)
        ((acc - target.cuda()) ** 2).mean().backward()
    assert _rel_l2(acc.detach().cpu().numpy(), acc_want.numpy()) < 2e-6
    # 2e-4: an operand that sits on a bf16 rounding boundary may round the other way after an fp32 reordering (one 2^-9
    # flip among thousands of operands); a kernel that rounded in the wrong place would be off by ~4e-3
    for got, want in zip([l.weight.grad for l in net.layers], [dW0, dW1, dW2, dw3]):
        assert _rel_l2(got.cpu().numpy(), want.numpy()) < 2e-4
    # table gradient = scatter of the bf16-rounded feature gradients
    xn = ((pts + 0.3) / 0.6).numpy().astype(np.float32)
    offs = net.encoder.offsets.cpu().numpy()
    ge = hash_encode_backward(r(dx).numpy(), xn, offs, 16, int(offs[-1]), 2)
    assert _rel_l2(net.encoder.embeddings.grad.cpu().numpy(), ge) < 2e-4


def test_bf16_table_end_to_end():
    _abi, encoder, fused, network = _mods()
    net, ref = _naf_pair(seed=5)
    net.encoder.embeddings.data = net.encoder.embeddings.data.to(torch.bfloat16)
    ref.encoder.embeddings.data.copy_(net.encoder.embeddings.data.float().cpu())
    from oracle import render_ref as R
    S, n = 192, 40
    rays = _rays(n, seed=11)
    t_rand = torch.rand(n, S)
    with torch.no_grad():
        want = R.render(rays, ref, None, S, 0, True, 1 << 20, 0.0, t_rand=t_rand)["acc"].numpy()
    acc = fused.fused_render(rays.cuda(), net, S, True, t_rand=t_rand.cuda())
    assert _rel_l2(acc.detach().cpu().numpy(), want) < 1e-2
    acc.sum().backward()
    assert net.encoder.embeddings.grad.dtype == torch.bfloat16


@pytest.mark.parametrize("prec,S", [("f32", 192), ("f32", 50), ("bf16", 192), ("bf16", 37), ("bf16", 17), ("bf16", 70), ("bf16", 100)])
def test_per_sample_sigma_and_running_optical_depth(prec, S):
    """naf_render_forward_samples: sigma[r,s] and the wave-prefix-summed optical depth tau[r,s] = sum_{s' <= s} sigma * dist
    against the oracle's per-sample network output and a float64 cumulative sum (render.py:192-201).  The last assertion compares the
    bf16 kernel's two tile loops bit for bit: with per-sample outputs it evaluates the activation per tile, without them once per four
    tiles (lane group j keeps tile k0 + j) -- S = 17 / 37 / 70 / 100 / 192 are 2 / 3 / 5 / 7 / 12 tiles, every remainder mod 4."""
    from oracle import render_ref as R
    _abi, encoder, fused, network = _mods()
    net, ref = _naf_pair(seed=14)
    n = 41
    rays = _rays(n, seed=19)
    t_rand = torch.rand(n, S, generator=torch.Generator().manual_seed(10))
    with torch.no_grad():
        z = R.sample_depths(rays[:, 6:7], rays[:, 7:], S, True, t_rand)
        pts = R.points_on_rays(rays, z, ref.bound)
        sig_ref = ref(pts.reshape(-1, 3)).reshape(n, S)
        dist = torch.cat([z[:, 1:] - z[:, :-1], torch.full((n, 1), 1e-10)], -1) * rays[:, 3:6].norm(dim=-1, keepdim=True)
        tau_ref = torch.cumsum((sig_ref * dist).double(), -1)
    precision = _abi.F32 if prec == "f32" else _abi.BF16
    acc, sigma, tau = fused.render_samples(rays.cuda(), net, S, True, t_rand=t_rand.cuda(), mlp_precision=precision)
    tol = 1e-4 if prec == "f32" else 1e-2
    assert _rel_l2(sigma.cpu().numpy(), sig_ref.numpy()) < tol
    assert _rel_l2(tau.cpu().numpy(), tau_ref.numpy()) < tol
    # sigmoid output: the depth never decreases -- up to the rounding of a floating-point scan (neighbouring prefixes are
    # summed along different trees, like torch.cumsum on a GPU): an ulp or two of the running value
    assert bool((tau[:, 1:] >= tau[:, :-1] - 4e-7 * tau[:, -1:]).all())
    np.testing.assert_allclose(tau[:, -1].cpu().numpy(), acc.cpu().numpy(), rtol=2e-6)     # same terms, scan vs tree order
    only_acc = fused.render_samples(rays.cuda(), net, S, True, t_rand=t_rand.cuda(), mlp_precision=precision, want_sigma=False,
                                    want_depth=False)[0]
    assert torch.equal(only_acc, acc)


@pytest.mark.parametrize("perturb", [False, True])
def test_fine_depths_kernel_matches_oracle_weights_sample_pdf_and_sort(perturb):
    """naf_fine_depths (one wave per ray: weights, cdf by wave prefix sum, inverse-transform sampling, bitonic merge sort)
    against the oracle's raw2outputs weights + sample_pdf + torch.sort on the SAME coarse sigma (render.py:113-126,203-247)."""
    from oracle import render_ref as R
    _abi, encoder, fused, network = _mods()
    net, _ = _naf_pair(seed=15)
    n, S, NF = 37, 64, 48
    rays = _rays(n, seed=21)
    t_rand = torch.rand(n, S, generator=torch.Generator().manual_seed(11)) if perturb else None
    u = torch.rand(n, NF, generator=torch.Generator().manual_seed(12)) if perturb else None
    _, sigma, _ = fused.render_samples(rays.cuda(), net, S, perturb, t_rand=None if t_rand is None else t_rand.cuda())
    z_all, w0 = fused.fine_depths(rays.cuda(), sigma, NF, perturb, t_rand=None if t_rand is None else t_rand.cuda(),
                                  u=None if u is None else u.cuda(), det=not perturb)
    z = R.sample_depths(rays[:, 6:7], rays[:, 7:], S, perturb, t_rand)
    _, weights = R.raw2outputs(sigma.cpu()[..., None], z, rays[:, 3:6], 0.0)
    mid = 0.5 * (z[:, 1:] + z[:, :-1])
    zs = R.sample_pdf(mid, weights[:, 1:-1], NF, det=not perturb, u=u)
    want = torch.sort(torch.cat([z, zs], -1), -1).values
    assert z_all.shape == (n, S + NF)
    np.testing.assert_allclose(w0.cpu().numpy(), weights.numpy(), rtol=1e-6, atol=1e-12)
    # the cdf is summed in scan order here and sequentially in torch: a few ulps of a depth of order 1 m
    np.testing.assert_allclose(z_all.cpu().numpy(), want.numpy(), rtol=0, atol=3e-6)
    assert bool((z_all[:, 1:] >= z_all[:, :-1]).all())


def test_fine_depths_single_fine_sample_det():
    """n_fine = 1 without jitter: torch.linspace(0, 1, 1) is [0] (render.py:224), so the one fine sample sits on the first bin
    edge -- the mid-point of the first two coarse depths (a 0 / 0 in the kernel's own linspace until round 2)."""
    _abi, encoder, fused, network = _mods()
    net, _ = _naf_pair(seed=15)
    n, S = 9, 12
    rays = _rays(n, seed=3).cuda()
    _, sigma, _ = fused.render_samples(rays, net, S, False)
    z_all, _ = fused.fine_depths(rays, sigma, 1, False, det=True)
    assert z_all.shape == (n, S + 1) and bool(torch.isfinite(z_all).all())
    z = torch.stack([rays[:, 6] + (rays[:, 7] - rays[:, 6]) * t for t in torch.linspace(0, 1, S).tolist()], 1)
    want = torch.sort(torch.cat([z, 0.5 * (z[:, :1] + z[:, 1:2])], 1), 1).values
    np.testing.assert_allclose(z_all.cpu().numpy(), want.cpu().numpy(), rtol=0, atol=2e-6)


def test_fused_coarse_to_fine_render_matches_oracle():
    """render(..., net_fine, n_fine > 0) with both networks in the fused shape: coarse forward with per-sample sigma ->
    naf_fine_depths -> fine render at the explicit depths (NAF_CFG_EXPLICIT_DEPTHS), against the oracle's render_chunk;
    gradients reach the fine network only (the fine depths are detached, render.py:121).

    The finest cells of the grid are 1.1 micrometres wide, so the fine network's features (random +-0.5 table here) change
    completely when a depth moves by one ulp: the resampled depths are therefore checked against the oracle's on their own
    (3e-6 m, also test_fine_depths_kernel_...), and the fine render and its gradients against the oracle evaluated AT those
    depths, where they must agree to fp32 rounding."""
    from neuralvolumetricreconstructionformedicalimages_amd import render as RR
    from oracle import render_ref as R
    _abi, encoder, fused, network = _mods()
    net, ref = _naf_pair(seed=16)
    net_fine, ref_fine = _naf_pair(seed=17)
    n, S, NF = 29, 48, 40
    rays = _rays(n, seed=23)
    target = torch.rand(n, generator=torch.Generator().manual_seed(13)) * 0.3
    with torch.no_grad():
        want = R.render(rays, ref, ref_fine, S, NF, False, 1 << 20, 0.0)
    got = RR.render(rays.cuda(), net, net_fine, S, NF, False, 4096, 0.0)
    assert set(got) >= {"acc", "acc0", "weights0", "pts0", "pts", "tv_loss"}
    assert _rel_l2(got["acc0"].cpu().numpy(), want["acc0"].numpy()) < 1e-4
    np.testing.assert_allclose(got["weights0"].cpu().numpy(), want["weights0"].numpy(), rtol=0, atol=1e-5)
    np.testing.assert_allclose(got["pts"].cpu().numpy(), want["pts"].numpy(), rtol=0, atol=5e-6)      # same resampled depths
    assert _rel_l2(got["acc"].detach().cpu().numpy(), want["acc"].numpy()) < 1e-3
    # the depths the fused path rendered at (deterministic: perturb = False), then the oracle's fine pass at exactly those
    _, sigma, _ = fused.render_samples(rays.cuda(), net, S, False)
    z_all, _ = fused.fine_depths(rays.cuda(), sigma, NF, False, det=True)
    np.testing.assert_allclose(_points_of(rays, z_all.cpu()), got["pts"].cpu().numpy(), rtol=0, atol=2e-7)
    zz = z_all.cpu()
    raw = R.run_network(R.points_on_rays(rays, zz, ref_fine.bound), ref_fine, 1 << 20)
    acc_ref, _ = R.raw2outputs(raw, zz, rays[:, 3:6], 0.0)
    ((acc_ref - target) ** 2).mean().backward()
    ((got["acc"] - target.cuda()) ** 2).mean().backward()
    assert _rel_l2(got["acc"].detach().cpu().numpy(), acc_ref.detach().numpy()) < 1e-4
    for a, b in zip(net_fine.layers, ref_fine.layers):
        assert _rel_l2(a.weight.grad.cpu().numpy(), b.weight.grad.numpy()) < 2e-4
    assert _rel_l2(net_fine.encoder.embeddings.grad.cpu().numpy(), ref_fine.encoder.embeddings.grad.numpy()) < 2e-4
    assert net.encoder.embeddings.grad is None                     # the coarse network only steers the sampling


def _points_of(rays, z):
    pts = rays[:, None, :3] + rays[:, None, 3:6] * z[:, :, None]
    return pts.clamp(-(0.3 - 1e-6), 0.3 - 1e-6).numpy()


def test_field_query_matches_oracle_and_unfused():
    _abi, encoder, fused, network = _mods()
    net, ref = _naf_pair(seed=6)
    pts = (torch.rand(5, 7, 11, 3) - 0.5) * 0.59
    with torch.no_grad():
        want = ref(pts.reshape(-1, 3)).reshape(5, 7, 11, 1).numpy()
        got = net(pts.cuda()).cpu().numpy()                         # fused: naf_field_forward
    np.testing.assert_allclose(got, want, rtol=2e-5, atol=1e-6)
    with torch.enable_grad():
        unf = net(pts.cuda()).detach().cpu().numpy()                # grad mode -> HIP encoder + rocBLAS Linear
    np.testing.assert_allclose(unf, want, rtol=2e-5, atol=1e-6)
    with pytest.raises(ValueError):
        with torch.no_grad():
            net(torch.tensor([[0.0, 0.31, 0.0]], device="cuda"))


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_generated_grid_query_is_bit_identical_to_the_point_list_query(prec):
    """naf_field_forward_grid (the voxel grid of tigre.py:388-400 generated inside the kernel, walked along x) against
    naf_field_forward on the materialised float32 point list: the same bits, for a non-cubic grid."""
    from neuralvolumetricreconstructionformedicalimages_amd.geometry import ConeGeometry, get_voxels
    from neuralvolumetricreconstructionformedicalimages_amd import phantom
    _abi, encoder, fused, network = _mods()
    net, ref = _naf_pair(seed=18)
    if prec == "bf16":
        net.encoder.embeddings.data = net.encoder.embeddings.data.to(torch.bfloat16)
    data = phantom.scan_geometry(64, "cone")
    data["nVoxel"], data["dVoxel"] = [37, 20, 51], [5.0, 9.0, 3.5]
    geo = ConeGeometry(data)
    vox = torch.tensor(get_voxels(geo), dtype=torch.float32, device="cuda")        # [37, 20, 51, 3] like TIGREDataset.voxels
    s = geo.sVoxel / 2 - geo.dVoxel / 2
    want = fused.field_query(net, vox).squeeze(-1)
    got = fused.field_query_grid(net, [-v for v in s], list(s), [37, 20, 51])
    assert got.shape == (37, 20, 51) and torch.equal(got, want)
    if prec == "f32":
        with torch.no_grad():
            oracle = ref(vox.cpu().reshape(-1, 3)).reshape(37, 20, 51)
        np.testing.assert_allclose(got.cpu().numpy(), oracle.numpy(), rtol=2e-5, atol=1e-6)
    with pytest.raises(ValueError):
        fused.field_query_grid(net, [-0.31, -0.1, -0.1], [0.3, 0.1, 0.1], [4, 4, 4])


def test_full_size_chest_batch_properties():
    """chest_50 sizes (T=2^19, S=192) at 4096 rays: fused == chunked fused (ray-order independence),
    constant table -> acc = sigma_const * path length, linearity of the table gradient in grad_acc."""
    _abi, encoder, fused, network = _mods()
    net, _ = _naf_pair(seed=7, log2T=19, scale=1e-4)
    n, S = 4096, 192
    rays = _rays(n, seed=13).cuda()
    t_rand = torch.rand(n, S, device="cuda")
    with torch.no_grad():
        full = fused.fused_render(rays, net, S, True, t_rand=t_rand)
        parts = torch.cat([fused.fused_render(rays[i:i + 1000], net, S, True, t_rand=t_rand[i:i + 1000]) for i in range(0, n, 1000)])
    assert torch.equal(full, parts)
    # constant table: every feature is the constant, sigma is one number, acc = sigma * sum(dist)
    with torch.no_grad():
        net.encoder.embeddings.fill_(0.25)
        sig = net(torch.zeros(1, 3, device="cuda")).item()
        acc = fused.fused_render(rays, net, S, False)
        z0, z1 = rays[:, 6], rays[:, 7]
        length = ((z1 - z0) + 1e-10) * rays[:, 3:6].norm(dim=-1)
    np.testing.assert_allclose(acc.cpu().numpy(), (sig * length).cpu().numpy(), rtol=2e-5)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_binned_scatter_equals_atomic_scatter(prec):
    """The two-pass binned gradient scatter (scatter_binned.h) against the reference-style atomic scatter on the same
    inputs, chest sizes (T=2^19, S=192, 2048 rays = 393k points -> 48 tiles x 16 levels x 256 buckets)."""
    _abi, encoder, fused, network = _mods()
    net, _ = _naf_pair(seed=8, log2T=19, scale=0.1)
    n, S = 2048, 192
    rays = _rays(n, seed=17).cuda()
    t_rand = torch.rand(n, S, device="cuda")
    target = torch.rand(n, device="cuda") * 0.3
    precision = _abi.F32 if prec == "f32" else _abi.BF16
    grads = {}
    for mode in (1, 2):
        with fused.scatter_mode(mode):
            net.zero_grad()
            acc = fused.fused_render(rays, net, S, True, t_rand=t_rand, mlp_precision=precision)
            ((acc - target) ** 2).mean().backward()
            grads[mode] = net.encoder.embeddings.grad.clone()
    a, b = grads[1].double(), grads[2].double()
    tol = 1e-5 if prec == "f32" else 3e-3          # bf16 records round each contribution once more (2^-9 relative)
    assert float((a - b).norm() / a.norm()) < tol
    assert float((a - b).abs().max() / a.abs().max()) < 10 * tol


def test_binned_scatter_large_batch_split_reducer():
    """2^18 rays x 128 samples = 33.5 M points: the record buffer holds 6 levels per pass, so the reducer splits every
    bucket's tiles between two workgroups (gridDim.z = 2, per-row atomics at the end).  Against the atomic scatter."""
    _abi, encoder, fused, network = _mods()
    net, _ = _naf_pair(seed=10, log2T=19, scale=0.1)
    n, S = 1 << 18, 128
    rays = _rays(n, seed=23).cuda()
    target = torch.rand(n, device="cuda") * 0.3
    grads = {}
    for mode in (1, 2):
        with fused.scatter_mode(mode):
            net.zero_grad()
            acc = fused.fused_render(rays, net, S, True, seed=3, mlp_precision=_abi.BF16)
            ((acc - target) ** 2).mean().backward()
            grads[mode] = net.encoder.embeddings.grad.clone()
    a, b = grads[1].double(), grads[2].double()
    assert float((a - b).norm() / a.norm()) < 3e-3
    assert float((a - b).abs().max() / a.abs().max()) < 3e-2


@pytest.mark.parametrize("log2T,n,S", [(16, 37, 50), (16, 41, 25), (20, 43, 97), (20, 64, 32), (21, 3, 683), (20, 1, 9)])
def test_binned_scatter_ragged_tail_tile_bf16(log2T, n, S):
    """Batches that end inside a pass-1 tile (1 024 points; 2 048 from T = 2^20 on, where pass 1 runs with 1 024 threads),
    fill it exactly (64 x 32 = 2 048), or are smaller than one tile: the threads past the end of the batch must contribute
    nothing, whatever the tile shape."""
    _abi, encoder, fused, network = _mods()
    net, _ = _naf_pair(seed=13, log2T=log2T, scale=0.1)
    rays = _rays(n, seed=41).cuda()
    t_rand = torch.rand(n, S, device="cuda")
    target = torch.rand(n, device="cuda") * 0.3
    grads = {}
    for mode in (1, 2):
        with fused.scatter_mode(mode):
            net.zero_grad()
            acc = fused.fused_render(rays, net, S, True, t_rand=t_rand, mlp_precision=_abi.BF16)
            ((acc - target) ** 2).mean().backward()
            grads[mode] = net.encoder.embeddings.grad.clone()
    a, b = grads[1].double(), grads[2].double()
    assert float((a - b).norm() / a.norm()) < 3e-3
    assert float((a - b).abs().max() / a.abs().max()) < 3e-2


def test_more_samples_than_the_lds_depth_buffer():
    """S = 1100 > 1024: the MLP kernels fall back from the per-ray LDS depth buffer to re-evaluating the depths."""
    from oracle import render_ref as R
    _abi, encoder, fused, network = _mods()
    net, ref = _naf_pair(seed=14)
    S, n = 1100, 5
    rays = _rays(n, seed=43)
    t_rand = torch.rand(n, S, generator=torch.Generator().manual_seed(2))
    target = torch.rand(n, generator=torch.Generator().manual_seed(3)) * 0.3
    acc_ref = R.render(rays, ref, None, S, 0, True, 1 << 20, 0.0, t_rand=t_rand)["acc"]
    ((acc_ref - target) ** 2).mean().backward()
    acc = fused.fused_render(rays.cuda(), net, S, True, t_rand=t_rand.cuda())
    ((acc - target.cuda()) ** 2).mean().backward()
    assert _rel_l2(acc.detach().cpu().numpy(), acc_ref.detach().numpy()) < 1e-4
    assert _rel_l2(net.encoder.embeddings.grad.cpu().numpy(), ref.encoder.embeddings.grad.numpy()) < 2e-4
    for a, b in zip(net.layers, ref.layers):
        assert _rel_l2(a.weight.grad.cpu().numpy(), b.weight.grad.numpy()) < 2e-4


def test_foot_config_t22_fp16_table_and_long_rays():
    """foot_50-like shapes (BASELINE.json configs[4]): T=2^22 (wrapped-dense fine levels, 512 scatter buckets), fp16
    table, S=320 -- forward vs the oracle, binned vs atomic gradient."""
    _abi, encoder, fused, network = _mods()
    from oracle import render_ref as R
    net, ref = _naf_pair(seed=9, log2T=22, scale=0.05)
    net.encoder.embeddings.data = net.encoder.embeddings.data.half()
    ref.encoder.embeddings.data.copy_(net.encoder.embeddings.data.float().cpu())
    S, n = 320, 24
    rays = _rays(n, seed=19)
    t_rand = torch.rand(n, S)
    with torch.no_grad():
        want = R.render(rays, ref, None, S, 0, True, 1 << 20, 0.0, t_rand=t_rand)["acc"].numpy()
    target = torch.rand(n, device="cuda") * 0.3
    grads = {}
    for mode in (1, 2):
        with fused.scatter_mode(mode):
            net.zero_grad()
            acc = fused.fused_render(rays.cuda(), net, S, True, t_rand=t_rand.cuda())
            (1e4 * (acc - target) ** 2).mean().backward()             # scaled: the gradient comes back in fp16 (table dtype)
            grads[mode] = net.encoder.embeddings.grad.float().clone()
    assert _rel_l2(acc.detach().cpu().numpy(), want) < 1e-2          # bf16 MFMA operands
    a, b = grads[1].double(), grads[2].double()
    assert float((a - b).norm() / a.norm()) < 5e-3                   # bf16 records + both rounded to fp16 at the end


def test_fine_pass_and_sample_pdf_match_reference_golden(golden):
    """Coarse + fine rendering (render.py:113-126, sample_pdf :215-247) on the drop-in surface vs the reference golden."""
    from neuralvolumetricreconstructionformedicalimages_amd import render as R
    _abi, encoder, fused, network = _mods()
    g = golden("render")
    net = _build_net(g)
    net_fine = network.DensityNetwork(net.encoder, bound=0.3, num_layers=4, hidden_dim=32, skips=[2], out_dim=1,
                                      last_activation="sigmoid").cuda()
    for i, lyr in enumerate(net_fine.layers):
        lyr.weight.data.copy_(torch.from_numpy(g[f"net_fine/w{i}"]))
        lyr.bias.data.copy_(torch.from_numpy(g[f"net_fine/b{i}"]))
    S = g["det/t_rand"].shape[1]
    with torch.no_grad():
        ret = R.render(torch.from_numpy(g["rays"]).cuda(), net, net_fine, S, 8, 0.0, 4096, 0.0)
    assert _rel_l2(ret["acc0"].cpu().numpy(), g["fine/acc0"]) < 1e-5
    np.testing.assert_allclose(ret["weights0"].cpu().numpy(), g["fine/weights0"], rtol=1e-4, atol=1e-6)
    assert _rel_l2(ret["acc"].cpu().numpy(), g["fine/acc"]) < 1e-4
    s = R.sample_pdf(torch.from_numpy(g["pdf/bins"]).cuda(), torch.from_numpy(g["pdf/weights"]).cuda(), 12, det=True)
    np.testing.assert_allclose(s.cpu().numpy(), g["pdf/samples_det"], rtol=1e-5)
    acc, w = R.raw2outputs(torch.from_numpy(g["r2o/raw"]).cuda(), torch.from_numpy(g["r2o/z"]).cuda(), torch.from_numpy(g["r2o/d"]).cuda())
    np.testing.assert_allclose(acc.cpu().numpy(), g["r2o/acc"], rtol=2e-6)
    np.testing.assert_allclose(w.cpu().numpy(), g["r2o/weights"], rtol=1e-6, atol=1e-12)


@pytest.mark.parametrize("case", range(10))
def test_fused_randomised_shapes_fp32_vs_oracle(case):
    """Seeded sweep over ray counts, sample counts, jitter on/off, table sizes, activations and both scatter paths:
    forward and every gradient of the fused fp32 path against the oracle."""
    from oracle import render_ref as R
    _abi, encoder, fused, network = _mods()
    rng = np.random.RandomState(1000 + case)
    n = int(rng.choice([1, 3, 17, 64, 130]))
    S = int(rng.choice([2, 7, 33, 64, 200, 321]))
    perturb = bool(rng.randint(2))
    log2T = int(rng.choice([8, 11, 14, 17]))
    act = str(rng.choice(["sigmoid", "relu", "tanh", "none"]))
    mode = int(rng.choice([1, 2]))
    net, ref = _naf_pair(seed=20 + case, log2T=log2T, last_activation=act)
    rays = _rays(n, seed=50 + case)
    gen = torch.Generator().manual_seed(70 + case)
    t_rand = torch.rand(n, S, generator=gen)
    target = torch.rand(n, generator=gen) * 0.3
    acc_ref = R.render(rays, ref, None, S, 0, perturb, 1 << 20, 0.0, t_rand=t_rand)["acc"]
    ((acc_ref - target) ** 2).mean().backward()
    with fused.scatter_mode(mode):
        acc = fused.fused_render(rays.cuda(), net, S, perturb, t_rand=t_rand.cuda())
        ((acc - target.cuda()) ** 2).mean().backward()
    tag = f"n={n} S={S} perturb={perturb} log2T={log2T} act={act} mode={mode}"
    assert _rel_l2(acc.detach().cpu().numpy(), acc_ref.detach().numpy()) < 1e-4, tag
    ge = ref.encoder.embeddings.grad.numpy()
    assert _rel_l2(net.encoder.embeddings.grad.cpu().numpy(), ge) < 3e-4, tag
    for a, b in zip(net.layers, ref.layers):
        gw = b.weight.grad.numpy()
        if np.abs(gw).max() > 0:
            assert _rel_l2(a.weight.grad.cpu().numpy(), gw) < 3e-4, tag

