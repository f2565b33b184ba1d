"""Every refusal of the stand-alone operators that is worded by a shared host helper (naf::fail_who, workspace_too_small, misaligned:
csrc/naf_host.h) keeps its return code and its whole text, and every entry point keeps its own order of refusals: where two could
apply, the case below names the one that wins.  The expected texts are the ones the entry points had when each formatted its own
message.  No GPU needed: every call returns before any launch."""
import ctypes

import pytest

P, Q, R, S = 4096, 8192, 12288, 16384          # four distinct pointers, aligned to anything asked for here
BIG = 1 << 30
FULL = 0xFFFFFFFF
HUGE = 1 << 20                                 # HUGE^3 voxels are 2^32 tiles of 8 x 32 columns


def _cases():
    from neuralvolumetricreconstructionformedicalimages_amd import _abi
    lib = _abi.lib()
    c = []

    def add(name, args, code, text):
        c.append((name, args, code, text))

    # ---- naf_tv_gradient(x, n1, n2, n3, eps, grad, stats, workspace, bytes, stream); (4, 9, 33) needs 4 blocks * 16 B -> 256 B
    # ---- naf_tv_descent(x, scratch, n1, n2, n3, step, n_steps, eps, stats, workspace, bytes, stream)
    def tv(who, n=(4, 9, 33), eps=1e-3, ws=S, size=BIG):
        if who == "tv_gradient":
            return "naf_tv_gradient", (P, *n, eps, Q, R, ws, size, None)
        return "naf_tv_descent", (P, Q, *n, 0.1, 2, eps, R, ws, size, None)

    for who in ("tv_gradient", "tv_descent"):
        add(*tv(who, n=(0, 9, 33)), -1, f"{who}: zero volume dimension")
        add(*tv(who, n=(4, 9, 0)), -1, f"{who}: zero volume dimension")
        add(*tv(who, eps=0.0), -1, f"{who}: eps must be > 0 and finite")
        add(*tv(who, eps=float("inf")), -1, f"{who}: eps must be > 0 and finite")
        add(*tv(who, n=(HUGE, HUGE, HUGE)), -1, f"{who}: volume too large for one call")
        add(*tv(who, size=255), -1, f"{who}: workspace too small (255 bytes, need 256)")
        add(*tv(who, size=0), -1, f"{who}: workspace too small (0 bytes, need 256)")
        add(*tv(who, ws=S + 4), -1, f"{who}: workspace must be 8-byte aligned")
        add(*tv(who, ws=S + 4, size=255), -1, f"{who}: workspace too small (255 bytes, need 256)")      # the size is looked at first
    add("naf_tv_gradient", (P, 4, 9, 33, 1e-3, Q, R, None, BIG, None), -1, "tv_gradient: null pointer")
    add("naf_tv_descent", (P, Q, 4, 9, 33, 0.1, 2, 1e-3, R, None, BIG, None), -1, "tv_descent: null pointer")

    # ---- naf_tv_prox_step(b, r, p, r_next, n1, n2, n3, lambda, momentum, nonneg, stream)
    # ---- naf_tv_prox_primal(b, p, x, n1, n2, n3, lambda, nonneg, stream)
    add("naf_tv_prox_step", (P, Q, R, S, 0, 9, 33, 1.0, 0.0, 0, None), -2, "tv_prox_step: zero volume dimension")
    add("naf_tv_prox_step", (P, Q, R, S, 4, 9, 0, 1.0, 0.0, 0, None), -2, "tv_prox_step: zero volume dimension")
    add("naf_tv_prox_step", (P, Q, R, S, HUGE, HUGE, HUGE, 1.0, 0.0, 0, None), -1, "tv_prox_step: volume too large for one call")
    add("naf_tv_prox_step", (P, Q, R, S, 0, 9, 33, 0.0, 0.0, 0, None), -2, "tv_prox_step: zero volume dimension")       # before lambda
    add("naf_tv_prox_primal", (P, Q, R, 4, 0, 33, 1.0, 0, None), -2, "tv_prox_primal: zero volume dimension")
    add("naf_tv_prox_primal", (P, Q, R, 65536, 65536, 1, 1.0, 0, None), -1, "tv_prox_primal: volume too large for one call")
    add("naf_tv_prox_primal", (P, Q, R, 0, 9, 33, -1.0, 0, None), -2, "tv_prox_primal: zero volume dimension")          # before lambda

    # ---- naf_ssim_3d(x, y, n1, n2, n3, out, workspace, bytes, stream); (7, 7, 7) is one window start: 1 block * 8 B -> 256 B
    def ssim(n=(7, 7, 7), ws=S, size=BIG):
        return "naf_ssim_3d", (P, Q, *n, R, ws, size, None)

    add(*ssim(size=255), -1, "ssim_3d: workspace too small (255 bytes, need 256)")
    add(*ssim(ws=S + 2), -1, "ssim_3d: workspace must be 8-byte aligned")
    add(*ssim(ws=S + 2, size=17), -1, "ssim_3d: workspace too small (17 bytes, need 256)")              # the size is looked at first
    add(*ssim(n=(6, 7, 7)), -1, "ssim_3d: win_size exceeds image extent (every extent must be >= 7, got 6 x 7 x 7)")
    add(*ssim(n=(HUGE, HUGE, HUGE)), -1, "ssim_3d: volume too large for one call")

    # ---- naf_cgls_wdot(a, w, n, slot, n_iter_max, workspace, bytes, stream); n = 100, 4 iterations: (32 scalars + 1 partial) * 8 B
    # ---- naf_cgls_residual_step(r, q, w, y, n, k, n_iter_max, workspace, bytes, stream)
    # ---- naf_cgls_direction_step(x, p, s, n, k, n_iter_max, workspace, bytes, stream)
    def cgls(who, ws=S, size=BIG, first=P):
        if who == "cgls_wdot":
            return "naf_cgls_wdot", (first, None, 100, 0, 4, ws, size, None)
        if who == "cgls_residual_step":
            return "naf_cgls_residual_step", (first, Q, None, R, 100, 0, 4, ws, size, None)
        return "naf_cgls_direction_step", (first, Q, R, 100, 0, 4, ws, size, None)

    for who in ("cgls_wdot", "cgls_residual_step", "cgls_direction_step"):
        add(*cgls(who, ws=None), -1, f"{who}: null pointer")
        add(*cgls(who, ws=S + 4), -1, f"{who}: workspace must be 8-byte aligned")
        add(*cgls(who, size=263), -1, f"{who}: workspace too small (263 bytes, need 264)")
        add(*cgls(who, ws=S + 4, size=263), -1, f"{who}: workspace must be 8-byte aligned")             # the alignment is looked at first
        add(*cgls(who, first=P + 2), -1, f"{who}: pointers must be 4-byte aligned")
        add(*cgls(who, first=P + 2, ws=S + 4, size=0), -1, f"{who}: pointers must be 4-byte aligned")   # the arrays before the workspace

    # ---- naf_resize_volume(in, in_dims, scale, shift, out, out_dims, minmax, workspace, bytes, stream)
    a, b = (ctypes.c_uint32 * 3)(5, 6, 7), (ctypes.c_uint32 * 3)(9, 4, 11)
    need = lib.naf_resize_volume_workspace_bytes(a, b)
    assert need > 0 and need % 16 == 0

    def resize(ws=S, size=BIG):
        return "naf_resize_volume", (P, a, 1.0, 0.0, Q, b, None, ws, size, None)

    add(*resize(size=need - 1), -1, f"resize_volume: workspace too small ({need - 1} bytes, need {need})")
    add(*resize(ws=S + 8), -1, "resize_volume: workspace must be 16-byte aligned")
    add(*resize(ws=S + 8, size=0), -1, f"resize_volume: workspace too small (0 bytes, need {need})")   # the size is looked at first
    add(*resize(ws=None), -1, "resize_volume: null pointer")

    # ---- naf_align_shift_scores(b, p, w, N, H, W, Rv, Ru, workspace, bytes, scores, stream); 1 view of 8 x 8, R = 1: 9 shifts * 1 tile * 8 B
    def scores(b=P, w=None, shape=(1, 8, 8), r=(1, 1), ws=S, size=BIG, out=R):
        return "naf_align_shift_scores", (b, Q, w, *shape, *r, ws, size, out, None)

    who = "align_shift_scores"
    add(*scores(ws=None), -1, f"{who}: null pointer")
    add(*scores(shape=(1, 0, 8)), -1, f"{who}: zero view dimension")
    add(*scores(shape=(1, 8, (1 << 24) + 1)), -1, f"{who}: view dimension above 2^24")
    add(*scores(r=(17, 1)), -1, f"{who}: max shift above 16")
    add(*scores(r=(4, 1)), -1, f"{who}: the search window needs 2 R < extent on each axis")
    add(*scores(b=P + 2), -1, f"{who}: views must be 4-byte aligned")
    add(*scores(w=R + 1), -1, f"{who}: views must be 4-byte aligned")
    add(*scores(ws=S + 4), -1, f"{who}: scores and workspace must be 8-byte aligned")
    add(*scores(out=R + 4), -1, f"{who}: scores and workspace must be 8-byte aligned")
    add(*scores(size=71), -1, f"{who}: workspace too small (71 bytes, need 72)")
    add(*scores(ws=S + 4, size=71), -1, f"{who}: scores and workspace must be 8-byte aligned")         # the alignment is looked at first
    add(*scores(shape=(FULL, 1 << 24, 1 << 24), r=(0, 0)), -1, f"{who}: too many tiles for one call")

    # ---- naf_align_peak(scores, N, Rv, Ru, shifts, flags, stream)
    add("naf_align_peak", (None, 2, 1, 1, Q, R, None), -1, "align_peak: null pointer")
    add("naf_align_peak", (P, 2, 1, 17, Q, R, None), -1, "align_peak: max shift above 16")
    add("naf_align_peak", (P, 0x80000000, 1, 1, Q, R, None), -1, "align_peak: too many views for one call")
    add("naf_align_peak", (P + 4, 2, 1, 1, Q, R, None), -1, "align_peak: misaligned pointer")
    add("naf_align_peak", (P, 2, 1, 1, Q + 2, R, None), -1, "align_peak: misaligned pointer")

    # ---- naf_align_shift_views(views, shifts, N, H, W, out, stream)
    who = "align_shift_views"
    add("naf_align_shift_views", (P, None, 2, 8, 8, R, None), -1, f"{who}: null pointer")
    add("naf_align_shift_views", (P, Q, 2, 0, 8, R, None), -1, f"{who}: zero view dimension")
    add("naf_align_shift_views", (P, Q, 2, 8, (1 << 24) + 1, R, None), -1, f"{who}: view dimension above 2^24")
    add("naf_align_shift_views", (P, Q, 2, 8, 8, P, None), -1, f"{who}: out must not be the views: every output pixel reads sixteen input pixels")
    add("naf_align_shift_views", (P, Q + 1, 2, 8, 8, R, None), -1, f"{who}: pointers must be 4-byte aligned")
    add("naf_align_shift_views", (P, Q, FULL, 1 << 24, 1 << 24, R, None), -1, f"{who}: too many pixels for one call")

    # ---- naf_stripe_remove_sorting(p, N, H, W, size, workspace, bytes, out, stream); a row of 3 views x 8 columns: 96 + 48 B
    def stripe(p=P, shape=(3, 4, 8), size=5, ws=S, ws_bytes=BIG, out=Q):
        return "naf_stripe_remove_sorting", (p, *shape, size, ws, ws_bytes, out, None)

    who = "stripe_remove_sorting"
    add(*stripe(out=None), -1, f"{who}: null pointer")
    add(*stripe(shape=(4097, 4, 8)), -1, f"{who}: more than 4096 views")
    add(*stripe(shape=(3, 4, (1 << 24) + 1)), -1, f"{who}: view dimension above 2^24")
    add(*stripe(size=4), -1, f"{who}: size must be odd and in [3, 63]")
    add(*stripe(size=9), -1, f"{who}: size above the number of detector columns")
    add(*stripe(p=P + 2), -1, f"{who}: projections must be 4-byte aligned")
    add(*stripe(ws=S + 4), -1, f"{who}: workspace must be 8-byte aligned")
    add(*stripe(ws_bytes=143), -1, f"{who}: workspace too small (143 bytes, one detector row needs 144)")
    add(*stripe(ws=S + 4, ws_bytes=143), -1, f"{who}: workspace must be 8-byte aligned")               # the alignment is looked at first

    # ---- naf_backproject_scan_gather(values, view_index, n_sub, n_scan_views, dims, dvoxel, poses, det, step, volume, den, workspace,
    #                                  bytes, stream); a view of 8 x 8 pixels has 64 spans of 40 B
    dims, dv = (ctypes.c_uint32 * 3)(4, 4, 4), (ctypes.c_float * 3)(1e-3, 1e-3, 1e-3)

    def gather(values=P, den=None, ws=None, size=0, du=1e-3):
        det = _abi.Detector(8, 8, du, 1e-3, 0.0, 0.0, 1.5, 0.0, 2.0, 0)
        return "naf_backproject_scan_gather", (values, None, 2, 2, dims, dv, Q, ctypes.byref(det), 5e-4, R, den, ws, size, None)

    who = "backproject_scan_gather"
    add(*gather(values=None), -1, f"{who}: null pointer")
    add(*gather(du=0.0), -1, f"{who}: pixel pitch must be finite and not 0")
    add(*gather(den=R), -1, f"{who}: volume and den must be two volumes")
    add(*gather(ws=S + 4, size=BIG), -1, f"{who}: workspace must be 8-byte aligned")
    add(*gather(ws=S, size=40 * 64 - 1), -1, f"{who}: workspace too small for the spans of one view")
    add(*gather(ws=S + 4, size=1), -1, f"{who}: workspace must be 8-byte aligned")                      # the alignment is looked at first

    # ---- naf_frames_condition(raw, raw_dtype, dark, flat, bad, N, H, W, size, dif, t_min, flags, out, counts, stream)
    def frames(raw=P, dtype=0, dark=Q, shape=(2, 8, 8), size=3, dif=0.1, t_min=1e-3, flags=0, out=S, counts=None):
        return "naf_frames_condition", (raw, dtype, dark, R, None, *shape, size, dif, t_min, flags, out, counts, None)

    who = "frames_condition"
    add(*frames(dark=None), -1, f"{who}: null pointer")
    add(*frames(dtype=2), -1, f"{who}: raw_dtype must be NAF_FRAMES_RAW_F32 or NAF_FRAMES_RAW_U16")
    add(*frames(size=4), -1, f"{who}: size must be 3, 5 or 7")
    add(*frames(raw=P + 2), -1, f"{who}: float32 raw must be 4-byte aligned")
    add(*frames(raw=P + 1, dtype=1), -1, f"{who}: uint16 raw must be 2-byte aligned")
    add(*frames(counts=S + 4098), -1, f"{who}: dark, flat, out and counts must be 4-byte aligned")
    add(*frames(raw=P + 2, dark=Q + 2), -1, f"{who}: float32 raw must be 4-byte aligned")              # raw before the other arrays
    add(*frames(out=P), -1, f"{who}: out must not overlap raw, dark, flat or bad")

    # ---- naf_render_train_adam(rays, t_rand, target, ray_weight, embeddings, offsets, mlp, acc, grad_embeddings, grad_mlp, loss_out,
    #                            n_rays, cfg, workspace, adam, stream): the checks of the Adam state come before everything else
    cfg = _abi.RenderCfg(n_samples=192, perturb=1, bound=0.3, L=16, C=2, H=16, table_dtype=2, mlp_precision=2, last_activation=0,
                         seed=0, ray_index_base=0, log2_hashmap_size=19)

    def train_adam(step=1, param=P, param_lp=None, lp_dtype=0):
        adam = _abi.TableAdam(param=param, exp_avg=Q, exp_avg_sq=R, param_lp=param_lp, lp_dtype=lp_dtype, n=1024, lr=1e-3, beta1=0.9,
                              beta2=0.999, eps=1e-8, step=step, grad_scale=1.0)
        return "naf_render_train_adam", (P, None, P, P, P, P, P, P, S, P, None, 8, ctypes.byref(cfg), P, ctypes.byref(adam), None)

    add(*train_adam(step=0), -1, "render_train_adam: step is 1-based")
    add(*train_adam(param_lp=S, lp_dtype=0), -2, "render_train_adam: lp_dtype must be NAF_F16 or NAF_BF16 when param_lp is given")
    add(*train_adam(param=P + 8), -1, "render_train_adam: buffers must be 16-byte aligned")
    add(*train_adam(step=0, param=P + 8), -1, "render_train_adam: step is 1-based")                     # the step is looked at first
    return c


ENTRY_POINTS = ("naf_tv_gradient", "naf_tv_descent", "naf_tv_prox_step", "naf_tv_prox_primal", "naf_ssim_3d", "naf_cgls_wdot",
                "naf_cgls_residual_step", "naf_cgls_direction_step", "naf_resize_volume", "naf_align_shift_scores", "naf_align_peak",
                "naf_align_shift_views", "naf_stripe_remove_sorting", "naf_backproject_scan_gather", "naf_frames_condition",
                "naf_render_train_adam")


@pytest.mark.parametrize("entry", ENTRY_POINTS)
def test_refusals_keep_their_code_and_their_whole_text(entry):
    from neuralvolumetricreconstructionformedicalimages_amd import _abi
    lib = _abi.lib()
    cases = [c for c in _cases() if c[0] == entry]
    assert len(cases) >= 3
    for name, args, code, text in cases:
        assert lib.naf_abi_version() == 6                                  # a call in between that leaves the last error alone
        got = getattr(lib, name)(*args)
        assert (got, lib.naf_last_error().decode()) == (code, text), args


def test_no_case_is_left_without_its_entry_point():
    assert {c[0] for c in _cases()} == set(ENTRY_POINTS)
