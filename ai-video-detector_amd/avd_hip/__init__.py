"""MI355X-native per-frame video analysis (hot path of backtato/ai-video-detector).

``avd_hip`` is the host side above the C-ABI of libavd_hip.so:
  _lib      ctypes binding (include/avd.h), fails loudly without the HIP extension
  timeline  float64 scalar tail of reference video.py:54-83 over per-frame records
  analyzer  FrameAnalyzer: frames -> records (HIP) -> result dict, chunked streaming;
            ClipsInFlight: several clips in flight on one GPU (service throughput mode);
            StreamMux: several live streams batched in one call per round (option "stream_map")
  sources   runtime-probed frame sources (decoders are optional host plumbing)
  dist      frame-parallel sharding across ranks + record all-gather (RCCL / gloo)
"""
from ._lib import AvdError, Context, Pixels, RECORD_DTYPE, build, load  # noqa: F401
from ._lib import AVD_FMT_BGR24, AVD_FMT_BGRA32, AVD_FMT_I420, AVD_FMT_NV12, AVD_FMT_RGB24, AVD_FMT_RGBA32, AVD_FMT_RGBP  # noqa: F401
from ._lib import AVD_FMT_I422, AVD_FMT_NV16, AVD_FMT_UYVY422, AVD_FMT_YUYV422  # noqa: F401
from ._lib import AVD_FMT_I010, AVD_FMT_P010  # noqa: F401
from ._lib import CV2_GAUSS_MULADD, CV2_RESIZE_LERP, CV2_THREE_SCALES  # noqa: F401
from .analyzer import ClipsInFlight, ContextPool, FrameAnalyzer, StreamMux, analyze_frames, default_pool  # noqa: F401
from .timeline import records_to_result, sample_step  # noqa: F401
