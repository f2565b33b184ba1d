"""MI355X-native Neural Attenuation Field hot path (hash-grid encoder, sigma-MLP, ray march, Adam) behind the
reference project's Python surface.  Compute lives in lib/libnaf_hip.so (hand-written HIP for gfx950, C ABI in
include/naf_hip.h); PyTorch-ROCm supplies device memory, streams and torch.distributed only."""

__version__ = "0.1.0"

from .volume import prepare_volume, resize_volume  # noqa: E402,F401
from .reconstruct import (align_operators, align_projections, asd_pocs, asd_pocs_operators, cgls, cgls_operators, fdk, fdk_operators, fista_tv, fista_tv_operators, os_sart,  # noqa: E402,F401
                          lamino_fbp, lamino_fbp_operators, os_sart_operators, reduce_metal, reduce_metal_operators, sirt, sirt_operators, subset_order)  # noqa: E402,F401
