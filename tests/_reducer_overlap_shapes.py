"""Shapes of tests/test_hip_reducer_overlap.py and a restatement of the launch plan they run under (not a test module).

The reducer of csrc/scatter_v2.h requests the Adam operands of a thread's late quads behind the wave's last record loads.  The shapes
are the smallest at which that order can go wrong; tests/test_reducer_overlap_plan_cpu.py checks without a GPU that each of them has the
property it is there for.  plan() restates make_bin_plan (csrc/scatter_host.h) for 8-byte records with the binned scatter forced,
level_layout() restates make_level_meta / make_row_map (csrc/naf_device.h, csrc/scatter_binned.h) and the reducer's own row
bookkeeping, wave_ranges() the tile range of each of the reducer's sixteen waves.

The engine takes the canonical network only (16 levels x 2 channels = the MLP's 32 inputs), so the shapes have L = 16: with base
resolution 4 and 2^14 rows the first four levels are 5^3, 9^3, 17^3 rows (dense) and 2^14 rows (hashed), the other twelve are
hashed too."""
import numpy as np

L, C, H, LOG2T = 16, 2, 4, 14
REDUCER_THREADS, WAVES = 1024, 16

# name -> rays, samples per ray, rows added to level 0 (shifts every later level's offset by one: the other parity), step with an
# infinite target (its feature gradients are not finite: the reducer poisons its sums) or None
SHAPES = {
    "a-small-dense-and-cut-chunks": dict(n=64, S=48, pad0=0, inf_step=None),
    "b-other-offset-parity": dict(n=64, S=48, pad0=1, inf_step=None),
    "c-ragged-tiles-idle-waves": dict(n=1001, S=16, pad0=0, inf_step=None),
    "d-non-finite-gradient": dict(n=64, S=48, pad0=0, inf_step=1),
}


def offsets(pad0=0):
    """Row offsets per level, int32 [L + 1] (encoder.level_offsets), level 0 padded by `pad0` rows it never uses."""
    sizes = [min(1 << LOG2T, (H * 2 ** l + 1) ** 3) for l in range(L)]
    sizes[0] += pad0
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def plan(n_points):
    """make_bin_plan for PairFx records (8 bytes: 512 threads x 2 points per tile), scatter_mode = binned, no flags."""
    log2_nb = 6
    while ((1 << LOG2T) >> log2_nb) * C * 8 > (128 << 10):
        log2_nb += 1
    tile = 512 * 2 * (2 if log2_nb >= 7 else 1)
    mean_run = max(1, (tile * 4) >> log2_nb)
    log2_w = 3
    while log2_w < 6 and (1 << log2_w) < mean_run + mean_run // 4:
        log2_w += 1
    return dict(tile_points=tile, n_tiles=(n_points + tile - 1) // tile, log2_nb=log2_nb, log2_w=log2_w,
                slots=min(65504, (tile * 11 // 2 + 31) & ~31), max_local_rows=((((1 << LOG2T) + (1 << log2_nb) - 1) >> log2_nb) + 63) & ~63)


def level_layout(offs, level, log2_nb):
    """What the reducer's workgroups of one level own: dict(T, offset, dense, s, rows_local, n_quads, buckets_with_rows)."""
    off, T = int(offs[level]), int(offs[level + 1] - offs[level])
    dense = (H * 2 ** level + 1) ** 3 <= T
    bits = (T - 1).bit_length() if T > 1 else 0
    sh = max(bits - log2_nb, 0)
    s = max(1, min(sh, 6) if dense else sh)
    hs = s + log2_nb
    rows_local = ((T + (1 << hs) - 1) >> hs) << s
    return dict(T=T, offset=off, dense=dense, s=s, hs=hs, rows_local=rows_local, n_quads=(rows_local + 1) >> 1,
                buckets_with_rows=sum(1 for b in range(1 << log2_nb) if (b << s) < T))


def owner(layout, rows, log2_nb):
    """(bucket, local row) of table rows of a level: RowMap::bucket, RowMap::local."""
    s, hs = layout["s"], layout["hs"]
    return (rows >> s) & ((1 << log2_nb) - 1), (rows & ((1 << s) - 1)) | ((rows >> hs) << s)


def wave_ranges(n_tiles):
    """[t_begin, t_end) of the reducer's waves in an unsplit launch (gridDim.z = 1)."""
    share = (n_tiles + WAVES - 1) // WAVES
    per_wave = (share + 63) & ~63 if share >= 64 else (share + 7) & ~7
    return [(w * per_wave, min(n_tiles, (w + 1) * per_wave)) for w in range(WAVES)]
