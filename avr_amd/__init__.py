"""avr_amd — MI355X-native acoustic volume renderer (hot path of KMASAHIRO/AVR).

`AVRRender` is a drop-in for the reference's `renderer.AVRRender`; the render
core, ray generation, sampling, hash-grid encoding and IR synthesis run in
hand-written HIP kernels for gfx950 behind the C-ABI in `include/avr_hip.h`.
"""
from .renderer import (  # noqa: F401
    AVRRender,
    RenderCore,
    RenderCoreMC,
    denormalize_points,
    normalize_points,
    ray_directions,
    sh_decode,
    spectrum_to_ir,
)
from .criterion import Criterion  # noqa: F401
from .metrics import (  # noqa: F401
    MetricAccumulator,
    calculate_metrics,
    metric_cal,
    metric_rows,
)
from .auralize import (  # noqa: F401
    auralize_dump,
    auralize_path,
    butter_bandpass_sos,
    convolve_source,
    convolve_trajectory,
    seg_hop_samples,
    sliding_frames,
    sosfilt_zi,
    synth_observation,
    synth_trajectory,
    trajectory_weights,
    white_noise,
    zero_phase_sos,
)
from .doa import (  # noqa: F401
    das_doa,
    das_doa_dump,
    doa_bins,
    doa_frames,
    frame_stats,
)
from .options import KernelOptions  # noqa: F401
from . import spatial  # noqa: F401
from . import workloads  # noqa: F401

__version__ = "0.1.0"
