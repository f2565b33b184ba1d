// abi_layout_host_check.cpp -- what the C compiler makes of the public structs of include/naf_hip.h: for each of them one line
// "struct <name> <sizeof>" and then one line "field <name> <offsetof>" per field, in the header's order.  tools/abi_layout_host_check.py
// holds them against the ctypes mirrors of _abi.py and against the field names it reads from the header's text, so a field that is
// added, dropped or moved on any of the three sides shows.  The header and nothing of HIP.  No GPU.
#include <cstddef>
#include <cstdio>

#include "../include/naf_hip.h"

#define STRUCT(T) std::printf("struct %s %zu\n", #T, sizeof(T))
#define FIELD(T, f) std::printf("field %s %zu\n", #f, offsetof(T, f))

int main() {
    STRUCT(naf_render_cfg);
    FIELD(naf_render_cfg, n_samples);
    FIELD(naf_render_cfg, perturb);
    FIELD(naf_render_cfg, bound);
    FIELD(naf_render_cfg, L);
    FIELD(naf_render_cfg, C);
    FIELD(naf_render_cfg, H);
    FIELD(naf_render_cfg, table_dtype);
    FIELD(naf_render_cfg, mlp_precision);
    FIELD(naf_render_cfg, last_activation);
    FIELD(naf_render_cfg, seed);
    FIELD(naf_render_cfg, ray_index_base);
    FIELD(naf_render_cfg, log2_hashmap_size);
    FIELD(naf_render_cfg, scatter_mode);
    FIELD(naf_render_cfg, flags);

    STRUCT(naf_grad_buckets);
    FIELD(naf_grad_buckets, n_buckets);
    FIELD(naf_grad_buckets, level_begin);
    FIELD(naf_grad_buckets, level_end);
    FIELD(naf_grad_buckets, ready);
    FIELD(naf_grad_buckets, mlp_ready);

    STRUCT(naf_table_adam);
    FIELD(naf_table_adam, param);
    FIELD(naf_table_adam, exp_avg);
    FIELD(naf_table_adam, exp_avg_sq);
    FIELD(naf_table_adam, param_lp);
    FIELD(naf_table_adam, lp_dtype);
    FIELD(naf_table_adam, n);
    FIELD(naf_table_adam, lr);
    FIELD(naf_table_adam, beta1);
    FIELD(naf_table_adam, beta2);
    FIELD(naf_table_adam, eps);
    FIELD(naf_table_adam, step);
    FIELD(naf_table_adam, grad_scale);
    FIELD(naf_table_adam, mlp_param);
    FIELD(naf_table_adam, mlp_exp_avg);
    FIELD(naf_table_adam, mlp_exp_avg_sq);

    STRUCT(naf_scan_draw);
    FIELD(naf_scan_draw, n_segments);
    FIELD(naf_scan_draw, rays_per_segment);
    FIELD(naf_scan_draw, valid);
    FIELD(naf_scan_draw, n_valid);

    STRUCT(naf_detector);
    FIELD(naf_detector, det_w);
    FIELD(naf_detector, det_h);
    FIELD(naf_detector, du);
    FIELD(naf_detector, dv);
    FIELD(naf_detector, ou);
    FIELD(naf_detector, ov);
    FIELD(naf_detector, DSD);
    FIELD(naf_detector, near);
    FIELD(naf_detector, far);
    FIELD(naf_detector, parallel);

    STRUCT(naf_next_draw);
    FIELD(naf_next_draw, draw);
    FIELD(naf_next_draw, poses);
    FIELD(naf_next_draw, projections);
    FIELD(naf_next_draw, pixels);
    FIELD(naf_next_draw, target);
    FIELD(naf_next_draw, rays);
    FIELD(naf_next_draw, first_draw);
    FIELD(naf_next_draw, n_draws);
    FIELD(naf_next_draw, n_projections);
    FIELD(naf_next_draw, det);
    FIELD(naf_next_draw, seed);
    return 0;
}
