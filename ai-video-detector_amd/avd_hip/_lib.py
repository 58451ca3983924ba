"""ctypes binding of libavd_hip.so (C-ABI declared in include/avd.h).

The library is built in-tree by ``make -C ai-video-detector_amd/csrc`` (or
``__graft_entry__.build()``).  There is no CPU fallback: if the shared object is
missing, or no HIP device is usable, loading / context creation raises.
"""
from __future__ import annotations

import collections
import ctypes as C
import math
import os
import subprocess
import sys
import typing

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(_PKG, "csrc")
SO_PATH = os.path.join(_PKG, "lib", "libavd_hip.so")

AVD_MEM_HOST, AVD_MEM_DEVICE = 0, 1
SMALL, HASH = 320, 32

EXPORTS = (
    "avd_abi_version", "avd_create", "avd_destroy", "avd_last_error",
    "avd_preprocess_bgr", "avd_farneback_pairs", "avd_analyze_frames",
    "avd_analyze_frames_async", "avd_synchronize", "avd_analyze_batch", "avd_analyze_batch_async",
    "avd_wait_stream", "avd_release_workspace",
    "avd_preprocess_nv12", "avd_analyze_frames_nv12", "avd_analyze_frames_nv12_async",
    "avd_preprocess_i420", "avd_analyze_frames_i420", "avd_analyze_frames_i420_async",
    "avd_preprocess_picture", "avd_analyze_pictures", "avd_analyze_pictures_async",
    "avd_vit_set_weights", "avd_vit_patch_embed", "avd_audio_features", "avd_layernorm", "avd_softmax",
    "avd_cnn_param_counts", "avd_cnn_set_weights", "avd_cnn_forward", "avd_cnn_conv",
    "avd_comm_unique_id", "avd_comm_init", "avd_allgather_records", "avd_allgather_last_records",
    "avd_timer_start", "avd_timer_stop", "avd_set_option", "avd_get_option",
    "avd_set_profiling", "avd_stage_ms", "avd_kernel_ms", "avd_debug_fetch",
)

# the frame-list family (include/avd_frame_list.h, which avd.h includes): additive at ABI 3, declared and listed apart from the entry points of avd.h
LIST_EXPORTS = ("avd_preprocess_frame_list", "avd_analyze_frame_lists", "avd_analyze_frame_lists_async")

# numpy view of struct avd_audio_window (48 bytes)
AUDIO_WINDOW_DTYPE = np.dtype([("sumsq", "<f8"), ("sum_log", "<f8"), ("sum_mag", "<f8"), ("sum_fmag", "<f8"),
                               ("zero_cross", "<i4"), ("length", "<i4"), ("rolloff_index", "<i4"), ("nbins", "<i4")])

# numpy view of struct avd_frame_record (32 bytes)
RECORD_DTYPE = np.dtype([("lap_sum", "<i8"), ("lap_sumsq", "<i8"), ("flow_mean", "<f4"),
                         ("flow_var", "<f4"), ("ham", "<i4"), ("reserved", "<i4")])


def f32_to_bf16_bits(a: np.ndarray) -> np.ndarray:
    """float32 -> bf16 bit patterns (uint16), round to nearest even (finite inputs)."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_bits_to_f32(b: np.ndarray) -> np.ndarray:
    return (b.astype(np.uint32) << 16).view(np.float32)


class AvdClip(C.Structure):
    """struct avd_clip (include/avd.h): one clip of a batch, BGR (uv = NULL) or NV12."""
    _fields_ = [("data", C.c_void_p), ("uv", C.c_void_p), ("mem", C.c_int), ("n", C.c_int), ("h", C.c_int), ("w", C.c_int),
                ("row_stride", C.c_int64), ("frame_stride", C.c_int64), ("uv_row_stride", C.c_int64), ("uv_frame_stride", C.c_int64)]


AVD_FMT_BGR24, AVD_FMT_NV12, AVD_FMT_I420 = 0, 1, 2
AVD_FMT_FULL_RANGE = 0x100      # flag OR-ed into a 4:2:0 layout: the samples use 0 .. 255 (ffmpeg's yuvj420p)
# what RGB producers hand over (include/avd.h): R,G,B interleaved; B,G,R,x and R,G,B,x with an ignored fourth byte; three planes R, G, B
AVD_FMT_RGB24, AVD_FMT_BGRA32, AVD_FMT_RGBA32, AVD_FMT_RGBP = 0x10, 0x11, 0x12, 0x13
# 4:2:2 (include/avd.h): Y0 U Y1 V and U Y0 V Y1 packed, 2 bytes per pixel; planar Y, U, V with chroma planes [H][W/2]; Y and interleaved U,V [H][W]
AVD_FMT_YUYV422, AVD_FMT_UYVY422, AVD_FMT_I422, AVD_FMT_NV16 = 0x20, 0x21, 0x22, 0x23
# 10-bit 4:2:0 in little-endian 16-bit words (include/avd.h): P010 = NV12's planes with the 10 bits in the high bits, I010 = I420's with them in the low bits
AVD_FMT_P010, AVD_FMT_I010 = 0x30, 0x31
# bits of option "cv2_model" (include/avd.h), the values of the oracle's own switches (the same numbers in its header): mul + add Gaussian taps, three pyramid
# scales, the 32f linear resize as a + (b - a) * f
CV2_GAUSS_MULADD, CV2_THREE_SCALES, CV2_RESIZE_LERP = 1, 8, 16
# One record per layout (csrc/avd_ingest_clip.h has the library's row; tests/test_ingest_layouts.py holds the two against include/avd.h).
#   px: bytes per pixel of plane 0; item: bytes per sample (2: planes of uint16 -- torch: uint16, or int16 read as the same bits; every stride
#   handed on is in bytes); planes 1 and 2 have H // ydiv rows of W // xdiv samples
#   handed: how a clip is handed over -- "stack": one interleaved array [N,H,W,px]; "channels": one array [N,3,H,W]; "planes": a tuple of planes
#   pixels: the clip goes through Pixels (an untagged array remains BGR24, untagged tuples remain NV12 / I420)
_Layout = collections.namedtuple("_Layout", "value name planes px item ydiv xdiv handed pixels")
LAYOUTS = (
    _Layout(AVD_FMT_BGR24, "AVD_FMT_BGR24", 1, 3, 1, 1, 1, "stack", True),
    _Layout(AVD_FMT_NV12, "AVD_FMT_NV12", 2, 1, 1, 2, 1, "planes", False),
    _Layout(AVD_FMT_I420, "AVD_FMT_I420", 3, 1, 1, 2, 2, "planes", False),
    _Layout(AVD_FMT_RGB24, "AVD_FMT_RGB24", 1, 3, 1, 1, 1, "stack", True),
    _Layout(AVD_FMT_BGRA32, "AVD_FMT_BGRA32", 1, 4, 1, 1, 1, "stack", True),
    _Layout(AVD_FMT_RGBA32, "AVD_FMT_RGBA32", 1, 4, 1, 1, 1, "stack", True),
    _Layout(AVD_FMT_RGBP, "AVD_FMT_RGBP", 3, 1, 1, 1, 1, "channels", True),
    _Layout(AVD_FMT_YUYV422, "AVD_FMT_YUYV422", 1, 2, 1, 1, 1, "stack", True),
    _Layout(AVD_FMT_UYVY422, "AVD_FMT_UYVY422", 1, 2, 1, 1, 1, "stack", True),
    _Layout(AVD_FMT_I422, "AVD_FMT_I422", 3, 1, 1, 1, 2, "planes", True),
    _Layout(AVD_FMT_NV16, "AVD_FMT_NV16", 2, 1, 1, 1, 1, "planes", True),
    _Layout(AVD_FMT_P010, "AVD_FMT_P010", 2, 2, 2, 2, 1, "planes", True),
    _Layout(AVD_FMT_I010, "AVD_FMT_I010", 3, 2, 2, 2, 2, "planes", True),
)
LAYOUT = {l.value: l for l in LAYOUTS}
_PACKED = {l.value: l.px for l in LAYOUTS if l.handed == "stack"}      # one interleaved plane: bytes per pixel
_WIDE = tuple(l.value for l in LAYOUTS if l.item == 2)


def _names(layouts) -> str:
    names = [l.name for l in layouts]
    return ", ".join(names[:-1]) + " or " + names[-1]


_FMT_NAMES = _names(LAYOUTS)


def _wide_dtype(p) -> bool:
    """is p a plane of 16-bit words: numpy uint16, torch uint16 or int16 (the same bits)"""
    return str(getattr(p, "dtype", None)) in ("uint16", "torch.uint16", "torch.int16")


def _chroma_shape(l: _Layout, h: int, w: int):
    """rows and samples per row of a plane behind plane 0: 4:2:0 halves the rows, the planar YUV layouts halve the row"""
    return (h // l.ydiv, w // l.xdiv)


class Pixels:
    """A clip tagged with its layout, accepted wherever a clip is (preprocess_picture, analyze_pictures, analyze_pictures_async):
    data uint8[N,H,W,3] for AVD_FMT_RGB24 (and AVD_FMT_BGR24), uint8[N,H,W,4] for AVD_FMT_BGRA32 / AVD_FMT_RGBA32, uint8[N,3,H,W] for
    AVD_FMT_RGBP (channels first, R,G,B: what torchcodec and torchvision.io decode to), uint8[N,H,W,2] for the packed 4:2:2 layouts
    AVD_FMT_YUYV422 / AVD_FMT_UYVY422; a tuple of planes for AVD_FMT_I422 (y uint8[N,H,W], u and v uint8[N,H,W/2]) and AVD_FMT_NV16
    (y, uv uint8[N,H,W]); a tuple of uint16 planes for the 10-bit layouts AVD_FMT_P010 (y uint16[N,H,W], uv uint16[N,H/2,W]: the 10 bits in the
    high bits) and AVD_FMT_I010 (y, u and v uint16[N,H/2,W/2]: in the low bits; a torch int16 tensor is read as the same bits); numpy or torch,
    host or device.  An untagged array remains BGR, untagged tuples remain NV12 / I420."""
    __slots__ = ("data", "fmt")

    def __init__(self, data, fmt: int):
        l = LAYOUT.get(fmt)
        if l is None or not l.pixels:
            raise ValueError(f"fmt must be {_names([l for l in LAYOUTS if l.pixels])}, got {fmt!r}")
        if l.handed == "planes":
            data = tuple(data)
            if len(data) != l.planes:
                raise ValueError(f"an {l.name} clip is a tuple of {l.planes} planes")
            if l.item == 2 and not all(_wide_dtype(p) for p in data):
                raise ValueError(f"the planes of an {l.name} clip are uint16 (torch: uint16 or int16), got {[str(getattr(p, 'dtype', type(p).__name__)) for p in data]}")
        self.data, self.fmt = data, fmt


class AvdPicture(C.Structure):
    """struct avd_picture (include/avd.h): one clip by descriptor -- BGR, NV12 or I420 planes of the STORED picture and the quarter turns
    (clockwise) that make it the displayed one."""
    _fields_ = [("struct_size", C.c_uint32), ("format", C.c_int32), ("plane", C.c_void_p * 3), ("row_stride", C.c_int64 * 3),
                ("frame_stride", C.c_int64 * 3), ("mem", C.c_int32), ("n", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
                ("rotate", C.c_int32), ("reserved", C.c_int32)]


class AvdFrameList(C.Structure):
    """struct avd_frame_list (include/avd_frame_list.h): one clip as a list of separately allocated frames -- per plane an array of n plane pointers (host
    memory, read during the call only) in place of avd_picture's base + f * frame_stride."""
    _fields_ = [("struct_size", C.c_uint32), ("format", C.c_int32), ("plane", C.c_void_p * 3), ("row_stride", C.c_int64 * 3),
                ("mem", C.c_int32), ("n", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("rotate", C.c_int32), ("reserved", C.c_int32)]


class AvdError(RuntimeError):
    """Non-zero status from the C-ABI (the analyzer may raise; reference api.py:134-140
    turns any exception into the neutral 0.5 timeline)."""


class _Clip(typing.NamedTuple):
    """One clip as the binding hands it to the library: planes are base pointers (BGR one, NV12 two, I420 three), rows / frames the byte
    strides, one per plane; keep is what the caller holds while the library reads the planes."""
    format: int
    planes: tuple
    mem: int
    n: int
    h: int
    w: int
    rows: tuple
    frames: tuple
    keep: object

    def args(self):
        """the leading arguments of the format's own C entry points (U and V of I420 share one pair of strides there)"""
        return self.planes + (self.mem, self.n, self.h, self.w) + self.rows[:2] + self.frames[:2]


def build(force: bool = False) -> str:
    """Compile the HIP extension for gfx950 with hipcc (cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp", ".h"))]
    srcs += [os.path.join(os.path.dirname(_PKG), "include", h) for h in ("avd.h", "avd_frame_list.h")]
    stale = (not os.path.exists(SO_PATH)) or any(os.path.getmtime(s) > os.path.getmtime(SO_PATH) for s in srcs)
    if force or stale:
        subprocess.run(["make", "-C", CSRC] + (["-B"] if force else []), check=True, stdout=sys.stderr)   # keep stdout clean (bench.py prints one JSON line)
    return SO_PATH


_lib = None


def _preload_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so (same SONAME as /opt/rocm's).
    Two HIP runtimes in one process cannot both own the GPU, and device pointers of torch
    tensors are only meaningful to the runtime that allocated them -- so when torch is
    installed, its runtime is loaded first and libavd_hip.so binds to it by SONAME."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return None
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        return C.CDLL(cand, mode=C.RTLD_GLOBAL)
    return None


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise ImportError(f"{SO_PATH} is missing: build it with `make -C {CSRC}` "
                          "(there is no CPU fallback for the HIP path)")
    _preload_hip_runtime()
    L = C.CDLL(SO_PATH)
    vp, u8p, f32p, i64p = C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p
    L.avd_abi_version.restype = C.c_int
    if L.avd_abi_version() != 3:          # before any other symbol is bound: an older library fails HERE, with a message
        raise ImportError("libavd_hip.so ABI version mismatch (this package binds version 3): rebuild it with `make -C csrc`")
    L.avd_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.avd_destroy.argtypes = [vp]
    L.avd_destroy.restype = None
    L.avd_last_error.argtypes = [vp]
    L.avd_last_error.restype = C.c_char_p
    L.avd_preprocess_bgr.argtypes = [vp, u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                     u8p, u8p, i64p, i64p]
    L.avd_farneback_pairs.argtypes = [vp, u8p, C.c_int, C.c_int, f32p, f32p, f32p]
    L.avd_analyze_frames.argtypes = [vp, u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, vp]
    L.avd_analyze_frames_async.argtypes = L.avd_analyze_frames.argtypes
    nv12 = [vp, u8p, u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64]
    L.avd_preprocess_nv12.argtypes = nv12 + [u8p, u8p, i64p, i64p]
    L.avd_analyze_frames_nv12.argtypes = nv12 + [vp]
    L.avd_analyze_frames_nv12_async.argtypes = nv12 + [vp]
    i420 = [vp, u8p, u8p, u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64]
    L.avd_preprocess_i420.argtypes = i420 + [u8p, u8p, i64p, i64p]
    L.avd_analyze_frames_i420.argtypes = i420 + [vp]
    L.avd_analyze_frames_i420_async.argtypes = i420 + [vp]
    L.avd_preprocess_picture.argtypes = [vp, vp, u8p, u8p, i64p, i64p]
    L.avd_analyze_pictures.argtypes = [vp, vp, C.c_int, vp]
    L.avd_analyze_pictures_async.argtypes = [vp, vp, C.c_int, vp]
    L.avd_preprocess_frame_list.argtypes = [vp, vp, u8p, u8p, i64p, i64p]
    L.avd_analyze_frame_lists.argtypes = [vp, vp, C.c_int, vp]
    L.avd_analyze_frame_lists_async.argtypes = [vp, vp, C.c_int, vp]
    L.avd_vit_set_weights.argtypes = [vp, vp, vp]
    L.avd_vit_patch_embed.argtypes = [vp, u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, vp, C.c_int, C.c_int, C.c_int,
                                      C.POINTER(C.c_float)]
    L.avd_cnn_param_counts.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.avd_cnn_set_weights.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t]
    L.avd_cnn_forward.argtypes = [vp, u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, vp, C.c_int, C.POINTER(C.c_float)]
    L.avd_cnn_conv.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
    L.avd_audio_features.argtypes = [vp, vp, C.c_int, C.c_int64, C.c_int, vp, C.c_int]
    L.avd_layernorm.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int64, C.c_int, vp, vp, C.c_float, vp, C.c_int, C.POINTER(C.c_float)]
    L.avd_softmax.argtypes = [vp, vp, C.c_int, C.c_int64, C.c_int, vp, C.c_int, C.POINTER(C.c_float)]
    L.avd_comm_unique_id.argtypes = [vp]
    L.avd_comm_init.argtypes = [vp, C.c_int, C.c_int, vp]
    L.avd_allgather_records.argtypes = [vp, vp, C.c_int, vp]
    L.avd_allgather_last_records.argtypes = [vp, C.c_int, vp]
    L.avd_synchronize.argtypes = [vp]
    L.avd_analyze_batch.argtypes = [vp, vp, C.c_int, vp]
    L.avd_analyze_batch_async.argtypes = [vp, vp, C.c_int, vp]
    L.avd_wait_stream.argtypes = [vp, vp]
    L.avd_release_workspace.argtypes = [vp]
    L.avd_timer_start.argtypes = [vp]
    L.avd_timer_stop.argtypes = [vp, C.POINTER(C.c_float)]
    L.avd_set_profiling.argtypes = [vp, C.c_int]
    L.avd_set_option.argtypes = [vp, C.c_char_p, C.c_int]
    L.avd_get_option.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int)]
    L.avd_stage_ms.argtypes = [vp, C.c_int, C.POINTER(C.c_float)]
    L.avd_kernel_ms.argtypes = [vp, C.c_int, C.POINTER(C.c_float)]
    L.avd_debug_fetch.argtypes = [vp, C.c_char_p, vp, C.c_size_t]
    L.avd_debug_fetch.restype = C.c_int64
    for name in EXPORTS + LIST_EXPORTS:
        if name not in ("avd_destroy", "avd_last_error", "avd_debug_fetch"):
            getattr(L, name).restype = C.c_int
    _lib = L
    return L


def _is_torch_tensor(x) -> bool:
    return type(x).__module__.startswith("torch") and hasattr(x, "data_ptr")


# what Context._plane_ptrs asks of a plane, whichever kind it is: (byte strides, base pointer, a dense copy)
_NUMPY_PLANE = (lambda a: a.strides, lambda a: a.ctypes.data, np.ascontiguousarray)
_TORCH_PLANE = (lambda t: t.stride(), lambda t: t.data_ptr(), lambda t: t.contiguous())


class Context:
    """One avd_ctx: one device, one HIP stream, one workspace.  Not re-entrant -- use one
    Context per thread (ctypes releases the GIL for the duration of each call)."""

    def __init__(self, device: int = 0):
        self._L = load()
        h = C.c_void_p()
        rc = self._L.avd_create(int(device), C.byref(h))
        if rc != 0 or not h:
            raise AvdError(f"avd_create(device={device}) failed with status {rc}: no usable HIP device "
                           "(the HIP path has no CPU fallback)")
        self._h = h
        self.device = int(device)
        self._list_keep = None          # the frames of a pending analyze_frame_lists_async, held until synchronize()

    def close(self):
        if getattr(self, "_h", None):
            self._L.avd_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc: int):
        if rc != 0:
            msg = self._L.avd_last_error(self._h)
            raise AvdError(f"avd status {rc}: {msg.decode() if msg else ''}")

    # -- buffers: numpy (host) or torch-ROCm tensors (device) ----------------------------
    def _after_torch_stream(self, t):
        """A device tensor may still be being written by torch's current stream (a fresh result, the copy kernel of
        ``.contiguous()``); the context launches on its own non-blocking stream, so order the two with an event
        (no host synchronisation).  The caller keeps the tensor alive until the work has been drained."""
        import torch
        if t.device.index is not None and t.device.index != self.device:
            raise ValueError(f"tensor lives on cuda:{t.device.index}, context on device {self.device}")
        self._check(self._L.avd_wait_stream(self._h, C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)))

    def _frames_ptr(self, frames):
        """-> (ptr, mem, n, h, w, row_stride, frame_stride, keepalive)"""
        if _is_torch_tensor(frames):
            t = frames
            if t.dim() != 4 or t.shape[-1] != 3 or str(t.dtype) != "torch.uint8":
                raise ValueError("frames must be uint8[N,H,W,3] (BGR)")
            n, h, w, _ = t.shape
            if t.stride(-1) != 1 or t.stride(-2) != 3 or t.stride(1) < 3 * w or (n > 1 and t.stride(0) < t.stride(1) * h):
                t = t.contiguous()
            mem = AVD_MEM_DEVICE if t.is_cuda else AVD_MEM_HOST
            if t.is_cuda:
                self._after_torch_stream(t)
            fs = t.stride(0) if n > 1 else h * t.stride(1)
            return t.data_ptr(), mem, n, h, w, t.stride(1), fs, t
        a = np.asarray(frames)
        if a.ndim != 4 or a.shape[-1] != 3 or a.dtype != np.uint8:
            raise ValueError("frames must be uint8[N,H,W,3] (BGR)")
        if a.strides[-1] != 1 or a.strides[-2] != 3 or a.strides[1] < a.shape[2] * 3 or (
                a.shape[0] > 1 and a.strides[0] < a.strides[1] * a.shape[1]):
            a = np.ascontiguousarray(a)
        n, h, w, _ = a.shape
        fs = a.strides[0] if n > 1 else h * a.strides[1]
        return a.ctypes.data, AVD_MEM_HOST, n, h, w, a.strides[1], fs, a

    def preprocess_bgr(self, frames):
        return self._preprocess("avd_preprocess_bgr", self._bgr(frames))

    def farneback_pairs(self, small, want_flow: bool = False):
        if _is_torch_tensor(small):
            t = small.contiguous()
            if t.is_cuda:
                self._after_torch_stream(t)
            ptr, mem, n, keep = t.data_ptr(), (AVD_MEM_DEVICE if t.is_cuda else AVD_MEM_HOST), t.shape[0], t
        else:
            a = np.ascontiguousarray(small, dtype=np.uint8)
            ptr, mem, n, keep = a.ctypes.data, AVD_MEM_HOST, a.shape[0], a
        m = max(n - 1, 0)
        fm = np.zeros(m, np.float32)
        fv = np.zeros(m, np.float32)
        flow = np.empty((m, SMALL, SMALL, 2), np.float32) if want_flow else None
        self._check(self._L.avd_farneback_pairs(self._h, ptr, mem, n, fm.ctypes.data, fv.ctypes.data,
                                                flow.ctypes.data if want_flow else None))
        return (fm, fv, flow) if want_flow else (fm, fv)

    def analyze_frames(self, frames) -> np.ndarray:
        """-> structured array (RECORD_DTYPE) with one record per frame."""
        return self._analyze("avd_analyze_frames", self._bgr(frames))

    # -- 4:2:0 planes.  NV12 (decoder surfaces): y uint8[N,H,W], uv uint8[N,H/2,W] with U,V interleaved.  I420 (planar, software decoders):
    # y uint8[N,H,W], u and v uint8[N,H/2,W/2]; YV12 = the same calls with u and v exchanged -------------------------------------------
    def _plane_ptrs(self, planes, fmt=None):
        """planes: an NV12 pair (y, uv) or an I420 triple (y, u, v), numpy or torch -> _Clip; fmt AVD_FMT_NV16 / AVD_FMT_I422: the same with
        chroma planes of H rows.  Strided views are passed
        as they are (a decoder's pitch, planes cut out of one buffer per clip); U and V must share their strides (the C-ABI has one pair for both)."""
        nv12 = len(planes) == 2
        if fmt is None:
            fmt = AVD_FMT_NV12 if nv12 else AVD_FMT_I420
        l = LAYOUT[fmt]
        ch = "H" if l.ydiv == 1 else "H/2"
        wide, item = l.item == 2, l.item                       # 16-bit words: the shapes count samples, the strides handed on are bytes
        ty = "uint16" if wide else "uint8"
        layout = f"{ty}[N,H,W] and {ty}[N,{ch},W]" if nv12 else f"{ty}[N,H,W], {ty}[N,{ch},W/2] and {ty}[N,{ch},W/2]"
        torch_in = [_is_torch_tensor(p) for p in planes]
        if any(torch_in) != all(torch_in):
            raise ValueError("both planes must be numpy arrays or both torch tensors" if nv12 else
                             "the three planes must all be numpy arrays or all torch tensors")
        if all(torch_in):
            cuda = planes[0].is_cuda
            if any(p.dim() != 3 or (not _wide_dtype(p) if wide else str(p.dtype) != "torch.uint8") or p.is_cuda != cuda for p in planes):
                raise ValueError(f"planes must be {layout} on the same device")
            _, ptr, dense = _TORCH_PLANE                       # torch's strides count elements
            strides = lambda t: tuple(v * item for v in t.stride())
        else:
            planes, cuda = tuple(np.asarray(p) for p in planes), False
            if any(p.ndim != 3 or p.dtype != (np.uint16 if wide else np.uint8) for p in planes):
                raise ValueError(f"planes must be {layout}")
            strides, ptr, dense = _NUMPY_PLANE
        st = []                                                # per plane: (row stride, frame stride) in bytes, as the library takes them
        for i, p in enumerate(planes):
            f, r, e = strides(p)
            if e != item or r < p.shape[2] * item or (p.shape[0] != 1 and f < r * p.shape[1]):
                p = dense(p)
                planes = planes[:i] + (p,) + planes[i + 1:]
                f, r, e = strides(p)
            st.append((r, f if p.shape[0] > 1 else p.shape[1] * r))
        n, h, w = (int(d) for d in planes[0].shape)
        got = [tuple(p.shape) for p in planes[1:]]
        crows, cbytes = _chroma_shape(l, h, w)
        if nv12 and got != [(n, crows, cbytes)]:
            raise ValueError(f"chroma plane must be {ty}[{n},{crows},{cbytes}] (interleaved U,V), got {got[0]}")
        if not nv12 and got != [(n, crows, cbytes)] * 2:
            raise ValueError(f"chroma planes must be {ty}[{n},{crows},{cbytes}] each, got {got[0]} and {got[1]}")
        if not nv12 and st[1] != st[2]:
            raise ValueError(f"the U and V planes must have the same row and frame strides, got {st[1]} and {st[2]}")
        if cuda:
            self._after_torch_stream(planes[0])
        return _Clip(fmt, tuple(ptr(p) for p in planes), AVD_MEM_DEVICE if cuda else AVD_MEM_HOST, n, h, w,
                     tuple(r for r, _ in st), tuple(f for _, f in st), planes)

    def _nv12_ptrs(self, y, uv):
        """-> (yptr, uvptr, mem, n, h, w, y_row, uv_row, y_frame, uv_frame, keepalive)"""
        c = self._plane_ptrs((y, uv))
        return c.args() + (c.keep,)

    def _i420_ptrs(self, y, u, v):
        """-> (yptr, uptr, vptr, mem, n, h, w, y_row, c_row, y_frame, c_frame, keepalive)"""
        c = self._plane_ptrs((y, u, v))
        return c.args() + (c.keep,)

    def _bgr(self, frames):
        ptr, mem, n, h, w, rs, fs, keep = self._frames_ptr(frames)
        return _Clip(AVD_FMT_BGR24, (ptr,), mem, int(n), int(h), int(w), (rs,), (fs,), keep)

    def _pixels(self, px):
        """A tagged clip (Pixels) -> _Clip.  A strided view goes through as it lies while its rows are dense (and, channels first, whatever the
        distance between the planes: they share their row and frame strides by construction); anything else is copied once, as _frames_ptr does."""
        fmt, l = px.fmt, LAYOUT[px.fmt]
        if fmt == AVD_FMT_BGR24:
            return self._bgr(px.data)
        if l.handed == "planes":
            return self._plane_ptrs(px.data, fmt)
        torch_in = _is_torch_tensor(px.data)
        a = px.data if torch_in else np.asarray(px.data)
        strides, ptr, dense = _TORCH_PLANE if torch_in else _NUMPY_PLANE
        planar = l.handed == "channels"
        want = "uint8[N,3,H,W] (R,G,B planes)" if planar else f"uint8[N,H,W,{l.px}]"
        shape = tuple(int(d) for d in a.shape)
        if len(shape) != 4 or shape[1 if planar else 3] != (3 if planar else l.px) or str(a.dtype) not in ("torch.uint8", "uint8"):
            raise ValueError(f"frames must be {want}, got {str(a.dtype)}{list(shape)}")
        n, h, w = (shape[0], shape[2], shape[3]) if planar else shape[:3]

        def lies_well(st):
            if planar:
                f, _, r, e = st
                return e == 1 and r >= w and (n <= 1 or f >= r * (h - 1) + w)
            f, r, p, e = st
            return e == 1 and p == l.px and r >= l.px * w and (n <= 1 or f >= r * h)
        if not lies_well(tuple(strides(a))):
            a = dense(a)
        st = tuple(int(v) for v in strides(a))
        row = st[2] if planar else st[1]
        frame = st[0] if n > 1 else h * row
        planes = tuple(ptr(a) + c * st[1] for c in range(3)) if planar else (ptr(a),)
        cuda = torch_in and a.is_cuda
        if cuda:
            self._after_torch_stream(a)
        return _Clip(fmt, planes, AVD_MEM_DEVICE if cuda else AVD_MEM_HOST, n, h, w, (row,) * len(planes), (frame,) * len(planes), a)

    def _clip(self, clip):
        """clip: a BGR frame stack uint8[N,H,W,3], an NV12 pair (y, uv), an I420 triple (y, u, v) or a tagged clip (Pixels); numpy or torch -> _Clip"""
        if isinstance(clip, Pixels):
            return self._pixels(clip)
        if not isinstance(clip, tuple):
            return self._bgr(clip)
        if len(clip) not in (2, 3):
            raise ValueError("a clip is a BGR frame stack, an NV12 pair (y, uv) or an I420 triple (y, u, v)")
        return self._plane_ptrs(clip)

    def _outputs_call(self, symbol, args, n):
        """An avd_preprocess_* call: the four host outputs of n frames behind `args`."""
        small = np.empty((n, SMALL, SMALL), np.uint8)
        hsh = np.empty((n, HASH * HASH), np.uint8)
        s = np.empty(n, np.int64)
        q = np.empty(n, np.int64)
        self._check(getattr(self._L, symbol)(self._h, *args, small.ctypes.data, hsh.ctypes.data, s.ctypes.data, q.ctypes.data))
        return small, hsh, s, q

    def _records_call(self, symbol, args, n, rec=None):
        """An avd_analyze_* call of n frames: blocking (rec None: a fresh record array is filled and returned) or asynchronous (the caller's
        rec is checked and handed over; synchronize() fills it)."""
        if rec is None:
            rec = np.zeros(n, RECORD_DTYPE)
        else:
            assert rec.dtype == RECORD_DTYPE and rec.size >= n and rec.flags.c_contiguous
        self._check(getattr(self._L, symbol)(self._h, *args, rec.ctypes.data))
        return rec

    def _preprocess(self, symbol, c):
        return self._outputs_call(symbol, c.args(), c.n)

    def _analyze(self, symbol, c, rec=None):
        """-> the records (blocking), or the buffers the kernels read (asynchronous: the caller holds them until synchronize())"""
        out = self._records_call(symbol, c.args(), c.n, rec)
        return out if rec is None else c.keep

    def preprocess_nv12(self, y, uv, rotate: int = 0, full_range: bool = False):
        """rotate: quarter turns clockwise from the stored planes to the displayed picture; full_range: the samples use 0 .. 255 (ffmpeg's J
        formats).  Either goes through the descriptor (avd_picture); without them this is the format's own entry point."""
        if rotate or full_range:
            return self.preprocess_picture((y, uv), rotate, full_range)
        return self._preprocess("avd_preprocess_nv12", self._plane_ptrs((y, uv)))

    def analyze_frames_nv12(self, y, uv, rotate: int = 0, full_range: bool = False) -> np.ndarray:
        if rotate or full_range:
            return self.analyze_pictures([(y, uv)], [rotate], [full_range])[0]
        return self._analyze("avd_analyze_frames_nv12", self._plane_ptrs((y, uv)))

    def analyze_frames_nv12_async(self, y, uv, rec: np.ndarray, rotate: int = 0, full_range: bool = False):
        if rotate or full_range:
            return self.analyze_pictures_async([(y, uv)], rec, [rotate], [full_range])[0][0]
        return self._analyze("avd_analyze_frames_nv12_async", self._plane_ptrs((y, uv)), rec)

    def preprocess_i420(self, y, u, v, rotate: int = 0, full_range: bool = False):
        if rotate or full_range:
            return self.preprocess_picture((y, u, v), rotate, full_range)
        return self._preprocess("avd_preprocess_i420", self._plane_ptrs((y, u, v)))

    def analyze_frames_i420(self, y, u, v, rotate: int = 0, full_range: bool = False) -> np.ndarray:
        if rotate or full_range:
            return self.analyze_pictures([(y, u, v)], [rotate], [full_range])[0]
        return self._analyze("avd_analyze_frames_i420", self._plane_ptrs((y, u, v)))

    def analyze_frames_i420_async(self, y, u, v, rec: np.ndarray, rotate: int = 0, full_range: bool = False):
        if rotate or full_range:
            return self.analyze_pictures_async([(y, u, v)], rec, [rotate], [full_range])[0][0]
        return self._analyze("avd_analyze_frames_i420_async", self._plane_ptrs((y, u, v)), rec)

    # -- pictures by descriptor (include/avd.h: avd_picture): any format, with a display rotation -------------------------------------------
    def _picture(self, clip, rotate: int = 0, full_range: bool = False):
        """clip: a BGR frame stack uint8[N,H,W,3], an NV12 pair (y, uv) or an I420 triple (y, u, v) of the STORED picture, or a tagged clip
        (Pixels: RGB, BGRA, RGBA, planar RGB, the four 4:2:2 layouts); numpy or torch.
        full_range: AVD_FMT_FULL_RANGE is OR-ed into the format (the library refuses it on BGR and RGB).
        -> (AvdPicture, frame count, keepalive).  The binding's own checks (the rotation, U and V of equal strides, planes all numpy or all
        torch) are made before the library is touched."""
        if isinstance(rotate, bool) or not isinstance(rotate, (int, np.integer)) or not 0 <= rotate <= 3:
            raise ValueError(f"rotate must be 0, 1, 2 or 3 quarter turns (clockwise, stored to displayed picture), got {rotate!r}")
        p = AvdPicture()
        p.struct_size, p.rotate, p.reserved = C.sizeof(AvdPicture), int(rotate), 0
        c = self._clip(clip)
        p.format, p.mem, p.n, p.h, p.w = c.format | (AVD_FMT_FULL_RANGE if full_range else 0), c.mem, c.n, c.h, c.w
        for i, plane in enumerate(c.planes):
            p.plane[i], p.row_stride[i], p.frame_stride[i] = plane, c.rows[i], c.frames[i]
        return p, c.n, c.keep

    def preprocess_picture(self, clip, rotate: int = 0, full_range: bool = False):
        """-> (small320, hash1024, lap_sum, lap_sumsq) of the DISPLAYED picture, as preprocess_bgr / _nv12 / _i420 on the turned planes;
        full_range: the 4:2:0 / 4:2:2 samples use 0 .. 255 and are converted as libswscale converts yuvj420p."""
        p, n, keep = self._picture(clip, rotate, full_range)
        return self._outputs_call("avd_preprocess_picture", (C.byref(p),), n)

    def _picture_array(self, clips, rotates, full_ranges=None):
        rotates = [0] * len(clips) if rotates is None else list(rotates)
        if len(rotates) != len(clips):
            raise ValueError("one rotation per clip")
        full_ranges = [False] * len(clips) if full_ranges is None else list(full_ranges)
        if len(full_ranges) != len(clips):
            raise ValueError("one range per clip")
        arr = (AvdPicture * len(clips))()
        keep, counts = [], []
        for i, (c, r, fr) in enumerate(zip(clips, rotates, full_ranges)):
            arr[i], n, k = self._picture(c, r, fr)
            keep.append(k)
            counts.append(n)
        return arr, counts, keep

    def analyze_pictures(self, clips, rotates=None, full_ranges=None):
        """A batch by descriptor: BGR stacks, NV12 pairs and I420 triples in any mix, each with its rotation (default 0) and its range
        (default limited; True = full range, 4:2:0 and 4:2:2 clips only).  -> list of record arrays, one per clip, identical to one call per clip."""
        arr, counts, keep = self._picture_array(clips, rotates, full_ranges)
        rec = self._records_call("avd_analyze_pictures", (arr, len(clips)), sum(counts))
        return list(np.split(rec, np.cumsum(counts)[:-1])) if counts else []

    def analyze_pictures_async(self, clips, rec: np.ndarray, rotates=None, full_ranges=None):
        """Enqueue only; rec (RECORD_DTYPE, sum of the clips' frames) is filled by synchronize().  Returns (keepalive, frame counts)."""
        arr, counts, keep = self._picture_array(clips, rotates, full_ranges)
        self._records_call("avd_analyze_pictures_async", (arr, len(clips)), sum(counts), rec)
        return keep, counts

    # -- clips as lists of separately allocated frames (include/avd_frame_list.h) ---------------------------------------------------------
    def _frame_list(self, frames, fmt: int, rotate: int = 0, full_range: bool = False):
        """frames: a sequence of per-frame arrays -- BGR or RGB uint8[H,W,3], BGRA / RGBA uint8[H,W,4], planar RGB uint8[3,H,W], NV12 pairs
        (y uint8[H,W], uv uint8[H/2,W]) or I420 triples (y, u, v), packed 4:2:2 uint8[H,W,2], I422 triples (y, u and v uint8[H,W/2]) or NV16
        pairs (y, uv uint8[H,W]) -- all
        numpy arrays (host) or all torch tensors on one device; every frame where it lies, nothing is gathered.  A plane's rows must be dense
        and all frames of the list share the row stride of each plane: anything else raises ValueError (there is no silent copy).
        -> (AvdFrameList, frame count, what the library reads: the pointer arrays during the call, the frames until it is drained)"""
        if isinstance(rotate, bool) or not isinstance(rotate, (int, np.integer)) or not 0 <= rotate <= 3:
            raise ValueError(f"rotate must be 0, 1, 2 or 3 quarter turns (clockwise, stored to displayed picture), got {rotate!r}")
        l = LAYOUT.get(fmt)
        if l is None:
            raise ValueError(f"fmt must be {_FMT_NAMES}, got {fmt!r}")
        nplanes, px, item, wide = l.planes, l.px, l.item, l.item == 2
        ty = "uint16" if wide else "uint8"
        if l.handed == "channels":                             # a [3,H,W] frame contributes its three channel views as planes
            frames = list(frames)
            for i, f in enumerate(frames):
                if len(getattr(f, "shape", ())) != 3 or int(f.shape[0]) != 3:
                    raise ValueError(f"frame {i}: an AVD_FMT_RGBP frame is uint8[3,H,W], got {list(getattr(f, 'shape', ()))}")
            frames = [(f[0], f[1], f[2]) for f in frames]
        else:
            frames = [(f,) if l.handed == "stack" else tuple(f) for f in frames]
        if any(len(f) != nplanes for f in frames):
            raise ValueError(f"every frame of the list has {nplanes} plane(s)")
        L = AvdFrameList()
        L.struct_size, L.format, L.rotate, L.reserved = C.sizeof(AvdFrameList), fmt | (AVD_FMT_FULL_RANGE if full_range else 0), int(rotate), 0
        L.n, L.mem = len(frames), AVD_MEM_HOST
        if not frames:                                         # an empty list has no picture to take a size from: any valid one
            L.h = L.w = HASH
            for p in range(nplanes):
                L.row_stride[p] = HASH * px if p == 0 else _chroma_shape(l, HASH, HASH)[1] * item
            return L, 0, ()
        torch_in = [_is_torch_tensor(p) for f in frames for p in f]
        if any(torch_in) != all(torch_in):
            raise ValueError("the frames of a list are all numpy arrays or all torch tensors")
        if all(torch_in):
            first = frames[0][0]
            if any((not _wide_dtype(p) if wide else str(p.dtype) != "torch.uint8") or p.device != first.device for f in frames for p in f):
                raise ValueError(f"the frames of a list are {ty} tensors on one device")
            _, ptr, _ = _TORCH_PLANE
            strides = lambda t: tuple(v * item for v in t.stride())      # torch counts elements, the library bytes
            if first.is_cuda:
                L.mem = AVD_MEM_DEVICE
                self._after_torch_stream(first)
        else:
            frames = [tuple(np.asarray(p) for p in f) for f in frames]
            if any(p.dtype != (np.uint16 if wide else np.uint8) for f in frames for p in f):
                raise ValueError(f"the frames of a list are {ty} arrays")
            strides, ptr, _ = _NUMPY_PLANE
        h, w = int(frames[0][0].shape[0]), int(frames[0][0].shape[1])
        shapes = [(h, w, px)] if l.handed == "stack" else [(h, w)] + [_chroma_shape(l, h, w)] * (nplanes - 1)
        arrays = []
        for p in range(nplanes):
            dense = (px, 1) if l.handed == "stack" else (item,)
            for i, f in enumerate(frames):
                if tuple(f[p].shape) != shapes[p]:
                    raise ValueError(f"frame {i}: plane {p} must be {ty}{list(shapes[p])}, got {list(f[p].shape)}")
                st = tuple(strides(f[p]))
                if st[1:] != dense:
                    raise ValueError(f"frame {i}: the rows of plane {p} are not dense (element strides {st[1:]})")
                if st[0] != strides(frames[0][p])[0]:
                    raise ValueError(f"frame {i}: plane {p} has row stride {st[0]}, frame 0 has {strides(frames[0][p])[0]}: the frames of a list share "
                                     "their row strides")
            L.row_stride[p] = int(strides(frames[0][p])[0])
            arrays.append((C.c_void_p * len(frames))(*[ptr(f[p]) for f in frames]))
            L.plane[p] = C.cast(arrays[-1], C.c_void_p)
        L.h, L.w = h, w
        return L, len(frames), (arrays, frames)

    def preprocess_frame_list(self, frames, fmt: int, rotate: int = 0, full_range: bool = False):
        """-> (small320, hash1024, lap_sum, lap_sumsq), as the format's own preprocess call on np.stack of the same frames."""
        L, n, keep = self._frame_list(frames, fmt, rotate, full_range)
        return self._outputs_call("avd_preprocess_frame_list", (C.byref(L),), n)

    def _frame_list_array(self, lists, rotates, full_ranges):
        rotates = [0] * len(lists) if rotates is None else list(rotates)
        full_ranges = [False] * len(lists) if full_ranges is None else list(full_ranges)
        if len(rotates) != len(lists) or len(full_ranges) != len(lists):
            raise ValueError("one rotation and one range per list")
        arr = (AvdFrameList * len(lists))()
        keep, counts = [], []
        for i, ((frames, fmt), r, fr) in enumerate(zip(lists, rotates, full_ranges)):
            arr[i], n, k = self._frame_list(frames, fmt, r, fr)
            keep.append(k)
            counts.append(n)
        return arr, counts, keep

    def analyze_frame_lists(self, lists, rotates=None, full_ranges=None):
        """lists: a sequence of (frames, fmt) -- frames as for preprocess_frame_list, any mix of formats and geometries, empty lists included --
        each with its rotation (default 0) and range (default limited).  -> list of record arrays, one per list, identical to the strided call
        on the stacked frames."""
        arr, counts, keep = self._frame_list_array(lists, rotates, full_ranges)
        rec = self._records_call("avd_analyze_frame_lists", (arr, len(lists)), sum(counts))
        self._list_keep = None                                 # a blocking call drains whatever was pending before it returns
        return list(np.split(rec, np.cumsum(counts)[:-1])) if counts else []

    def analyze_frame_lists_async(self, lists, rec: np.ndarray, rotates=None, full_ranges=None):
        """Enqueue only; rec (RECORD_DTYPE, sum of the lists' frames) is filled by synchronize().  Returns (keepalive, frame counts); the context
        itself also holds the frames until synchronize()."""
        arr, counts, keep = self._frame_list_array(lists, rotates, full_ranges)
        self._records_call("avd_analyze_frame_lists_async", (arr, len(lists)), sum(counts), rec)
        # only now: the C call above first drained a still-pending call, whose frames the context held until then
        self._list_keep = keep
        return keep, counts

    def ingest_list(self):
        """(1, frames) if the last ingest launch of this context took its frame bases from a table of plane pointers, else (0, 0);
        avd_debug_fetch "ingest_list"."""
        return tuple(int(v) for v in self.debug_fetch("ingest_list", (2,), np.int32))

    def stage_copies(self) -> int:
        """Host-to-device staging copies the last ingest call of this context issued; avd_debug_fetch "stage_copies"."""
        return int(self.debug_fetch("stage_copies", (1,), np.int64)[0])

    def ingest_format(self) -> int:
        """The layout (AVD_FMT_*) of the last ingest launch of this context; avd_debug_fetch "ingest_format"."""
        return int(self.debug_fetch("ingest_format", (1,), np.int32)[0])

    def ingest_rotate(self) -> int:
        """The rotation the last ingest launch of this context ran with; avd_debug_fetch "ingest_rotate"."""
        return int(self.debug_fetch("ingest_rotate", (1,), np.int32)[0])

    def ingest_range(self) -> int:
        """1 if the last ingest launch of this context ran with full-range conversion constants, else 0; avd_debug_fetch "ingest_range"."""
        return int(self.debug_fetch("ingest_range", (1,), np.int32)[0])

    def stage_bytes(self) -> int:
        """Bytes the last ingest call of this context copied from host memory (0: device input); avd_debug_fetch "stage_bytes"."""
        return int(self.debug_fetch("stage_bytes", (1,), np.int64)[0])

    # -- LayerNorm / softmax (extensions) -------------------------------------------------------------------------
    def layernorm(self, x, gamma, beta, eps: float = 1e-5, timing_reps: int = 0, out=None):
        """x: [rows, cols] float32 numpy array, or a contiguous float32 / bfloat16 torch-ROCm tensor (then ``out`` of the same
        kind receives the result in HBM, default: a new tensor).  -> (y, kernel_ms or None)"""
        g = np.ascontiguousarray(gamma, np.float32)
        b = np.ascontiguousarray(beta, np.float32)
        ms = C.c_float(0.0)
        if _is_torch_tensor(x):
            import torch
            if not (x.is_cuda and x.is_contiguous() and x.dim() == 2):
                raise ValueError("x must be a contiguous 2-D cuda tensor")
            bf = {"torch.float32": 0, "torch.bfloat16": 1}[str(x.dtype)]
            y = out if out is not None else torch.empty_like(x)
            self._after_torch_stream(x)
            self._check(self._L.avd_layernorm(self._h, x.data_ptr(), AVD_MEM_DEVICE, bf, x.shape[0], x.shape[1], g.ctypes.data, b.ctypes.data,
                                              eps, y.data_ptr(), timing_reps, C.byref(ms)))
            return y, (ms.value if timing_reps > 0 else None)
        a = np.ascontiguousarray(x, np.float32)
        y = np.empty_like(a)
        self._check(self._L.avd_layernorm(self._h, a.ctypes.data, AVD_MEM_HOST, 0, a.shape[0], a.shape[1], g.ctypes.data, b.ctypes.data, eps,
                                          y.ctypes.data, timing_reps, C.byref(ms)))
        return y, (ms.value if timing_reps > 0 else None)

    def softmax(self, x, timing_reps: int = 0):
        """x: [rows, cols] float32 (numpy or contiguous cuda tensor) -> (probabilities of the same kind, kernel_ms or None)"""
        ms = C.c_float(0.0)
        if _is_torch_tensor(x):
            import torch
            if not (x.is_cuda and x.is_contiguous() and x.dim() == 2 and str(x.dtype) == "torch.float32"):
                raise ValueError("x must be a contiguous 2-D float32 cuda tensor")
            y = torch.empty_like(x)
            self._after_torch_stream(x)
            self._check(self._L.avd_softmax(self._h, x.data_ptr(), AVD_MEM_DEVICE, x.shape[0], x.shape[1], y.data_ptr(), timing_reps, C.byref(ms)))
            return y, (ms.value if timing_reps > 0 else None)
        a = np.ascontiguousarray(x, np.float32)
        y = np.empty_like(a)
        self._check(self._L.avd_softmax(self._h, a.ctypes.data, AVD_MEM_HOST, a.shape[0], a.shape[1], y.ctypes.data, timing_reps, C.byref(ms)))
        return y, (ms.value if timing_reps > 0 else None)

    # -- ViT-B/16 patch embedding (extension, never part of ai_score) ------------------------------------------
    def vit_set_weights(self, weight: np.ndarray, bias=None):
        """weight float32[768, 768] ([out][c*256 + py*16 + px]) -> rounded to bf16 (nearest even); bias float32[768]."""
        wbits = f32_to_bf16_bits(np.ascontiguousarray(weight, np.float32).reshape(768, 768))
        b = None if bias is None else np.ascontiguousarray(bias, np.float32).reshape(768)
        self._check(self._L.avd_vit_set_weights(self._h, wbits.ctypes.data, None if b is None else b.ctypes.data))

    def vit_patch_embed(self, frames, timing_reps: int = 0, out=None, bf16: bool = False):
        """-> (tokens [N,196,768], gemm_ms or None).  Tokens are float32, or with ``bf16=True`` bf16 (returned to the host
        as float32 after widening).  ``out``: optional contiguous torch-ROCm tensor [N,196,768] (float32, or bfloat16 with
        ``bf16=True``) that receives the tokens in HBM (nothing is copied to the host then)."""
        ptr, mem, n, h, w, rs, fs, keep = self._frames_ptr(frames)
        ms = C.c_float(0.0)
        if out is not None:
            want = "torch.bfloat16" if bf16 else "torch.float32"
            if not (_is_torch_tensor(out) and out.is_cuda and out.is_contiguous() and tuple(out.shape) == (n, 196, 768)
                    and str(out.dtype) == want):
                raise ValueError(f"out must be a contiguous {want} cuda tensor [N,196,768]")
            self._after_torch_stream(out)
            tptr, tmem, tokens = out.data_ptr(), AVD_MEM_DEVICE, out
        else:
            tokens = np.empty((n, 196, 768), np.uint16 if bf16 else np.float32)
            tptr, tmem = tokens.ctypes.data, AVD_MEM_HOST
        self._check(self._L.avd_vit_patch_embed(self._h, ptr, mem, n, h, w, rs, fs, tptr, tmem, int(bool(bf16)), int(timing_reps), C.byref(ms)))
        if out is None and bf16:
            tokens = bf16_bits_to_f32(tokens)
        return tokens, (float(ms.value) if timing_reps > 0 else None)

    # -- CNN extension (ResNet-50-style forward on the matrix cores; never part of ai_score) -------------------------
    @staticmethod
    def cnn_param_counts():
        """-> (weights, biases): elements of the flat parameter arrays of avd_cnn_set_weights."""
        nw, nb = C.c_size_t(0), C.c_size_t(0)
        if load().avd_cnn_param_counts(C.byref(nw), C.byref(nb)) != 0:
            raise RuntimeError("avd_cnn_param_counts failed")
        return int(nw.value), int(nb.value)

    def cnn_set_weights(self, weights: np.ndarray, biases: np.ndarray):
        """weights: float32 flat (rounded to bf16, nearest even) or uint16 bf16 bits, in the order documented in avd.h."""
        w = np.ascontiguousarray(weights).reshape(-1)
        wbits = w if w.dtype == np.uint16 else f32_to_bf16_bits(w.astype(np.float32, copy=False))
        b = np.ascontiguousarray(biases, np.float32).reshape(-1)
        self._check(self._L.avd_cnn_set_weights(self._h, wbits.ctypes.data, wbits.size, b.ctypes.data, b.size))

    def cnn_forward(self, frames, timing_reps: int = 0):
        """-> (logits float32 [N,1000], forward_ms or None)."""
        ptr, mem, n, h, w, rs, fs, keep = self._frames_ptr(frames)
        logits = np.empty((n, 1000), np.float32)
        ms = C.c_float(0.0)
        self._check(self._L.avd_cnn_forward(self._h, ptr, mem, n, h, w, rs, fs, logits.ctypes.data, int(timing_reps), C.byref(ms)))
        return logits, (float(ms.value) if timing_reps > 0 else None)

    def cnn_conv(self, x: np.ndarray, w: np.ndarray, bias: np.ndarray, stride: int = 1, relu: bool = True, residual=None) -> np.ndarray:
        """One convolution layer (test entry).  x float32 NHWC [n,h,w,cin] and w float32 [cout,k,k,cin] are rounded to bf16;
        -> float32 NHWC (the widened bf16 output)."""
        n, hin, win, cin = x.shape
        cout, k, k2, cin2 = w.shape
        assert k == k2 and cin == cin2
        pad = k // 2
        hout, wout = (hin + 2 * pad - k) // stride + 1, (win + 2 * pad - k) // stride + 1
        xb = f32_to_bf16_bits(np.ascontiguousarray(x, np.float32))
        wb = f32_to_bf16_bits(np.ascontiguousarray(w, np.float32))
        b = np.ascontiguousarray(bias, np.float32)
        rb = None if residual is None else f32_to_bf16_bits(np.ascontiguousarray(residual, np.float32).reshape(n, hout, wout, cout))
        y = np.empty((n, hout, wout, cout), np.uint16)
        self._check(self._L.avd_cnn_conv(self._h, xb.ctypes.data, n, hin, win, cin, wb.ctypes.data, b.ctypes.data, cout, k, stride,
                                         int(bool(relu)), None if rb is None else rb.ctypes.data, y.ctypes.data))
        return bf16_bits_to_f32(y)

    @staticmethod
    def cnn_tap_shape(point: int, n: int):
        """-> (shape, dtype) of debug buffer "cnn_tap" after a forward of n frames under option cnn_tap = point: 1 the zero-bordered
        input image, 2 + i the output of convolution i (avd_cnn_set_weights order), 55 the max pool's output, 56 the pooled features."""
        if point == 1:
            return (n, 232, 232, 4), np.uint16
        if point == 55:
            return (n, 56, 56, 64), np.uint16
        if point == 56:
            return (n, 2048), np.float32
        outs = [(112, 64)]                                   # (side, channels) of every convolution's output, the stem first
        side = 56
        for st, depth in enumerate((3, 4, 6, 3)):
            mid = 64 << st
            for b in range(depth):
                so = side // 2 if (b == 0 and st > 0) else side
                outs += [(side, mid), (so, mid), (so, 4 * mid)] + ([(so, 4 * mid)] if b == 0 else [])
                side = so
        if not 2 <= point < 2 + len(outs):
            raise ValueError(f"cnn_tap point {point}")
        s, c = outs[point - 2]
        return (n, s, s, c), np.uint16

    def cnn_tap(self, n: int) -> np.ndarray:
        """What the last cnn_forward (of n frames) copied aside under option cnn_tap: bf16 bits (uint16) in NHWC, or float32 [n,2048]."""
        shape, dtype = self.cnn_tap_shape(self.get_option("cnn_tap"), n)
        return self.debug_fetch("cnn_tap", shape, dtype)

    def cnn_plan(self) -> np.ndarray:
        """int32[53]: the kernel shape each convolution of the last cnn_forward ran as (codes: avd.h, avd_debug_fetch "cnn_plan")."""
        return self.debug_fetch("cnn_plan", (53,), np.int32)

    # -- audio analyzer (reference app/analyzers/audio.py:40-61 for all windows at once) -----------------------
    @staticmethod
    def _is_pcm16(wav) -> bool:
        return str(wav.dtype) == "torch.int16" if _is_torch_tensor(wav) else getattr(wav, "dtype", None) == np.int16

    def _audio_ptr(self, wav, pcm16: bool):
        """-> (ptr, mem, n, keepalive) of mono samples: int16 PCM as it is (pcm16), anything else as float32"""
        if _is_torch_tensor(wav):
            t = wav.contiguous()
            if str(t.dtype) != ("torch.int16" if pcm16 else "torch.float32") or t.dim() != 1:
                raise ValueError("wav must be float32[n] or int16[n]")
            if t.is_cuda:
                self._after_torch_stream(t)
            return t.data_ptr(), (AVD_MEM_DEVICE if t.is_cuda else AVD_MEM_HOST), int(t.numel()), t
        a = np.ascontiguousarray(wav, dtype=np.int16 if pcm16 else np.float32)
        if a.ndim != 1:
            raise ValueError("wav must be float32[n] or int16[n]")
        return a.ctypes.data, AVD_MEM_HOST, int(a.size), a

    AUDIO_OUT_RATE = 16000
    AUDIO_RATES = (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000)

    @classmethod
    def audio_converted_length(cls, n: int, rate: int) -> int:
        """16 kHz output samples of a track of n frames at ``rate`` (option "audio_rate"): ceil(n * U / D)"""
        g = math.gcd(int(rate), cls.AUDIO_OUT_RATE)
        return -(-int(n) * (cls.AUDIO_OUT_RATE // g) // (int(rate) // g))

    def _audio_call(self, ptr, mem, n: int, win: int, nwin: int, pcm16: bool, cuts=(), rate=None, channels: int = 1, last: bool = False, entries=(),
                    layout: int = 0, stride: int = 0) -> np.ndarray:
        """One avd_audio_features call: option "audio_format" -- and, for a track at its decoder's rate, "audio_rate" and "audio_channels" -- set for
        it and restored (also after an exception), its cuts set in ascending order.  last: option "audio_end" is set for it (a slot call).
        entries: the "audio_track_slot" list of the call, set in track order and cleared if setting it fails (a call takes it whatever becomes of it).
        layout (an "audio_layout" value, not 0) and stride: options "audio_layout" / "audio_plane_stride" are set and restored the same way, in place
        of "audio_channels"; without a layout neither is touched."""
        out = np.zeros(nwin, AUDIO_WINDOW_DTYPE)
        if rate is not None and layout:
            was = self.get_option("audio_rate"), self.get_option("audio_layout"), self.get_option("audio_plane_stride")
            self.set_option("audio_rate", int(rate))          # a refused value leaves the options as they were: nothing has been set yet
            try:
                self.set_option("audio_layout", int(layout))
                self.set_option("audio_plane_stride", int(stride))
                return self._audio_call(ptr, mem, n, win, nwin, pcm16, cuts, None, 1, last, entries)
            finally:
                self.set_option("audio_rate", was[0])
                self.set_option("audio_layout", was[1])
                self.set_option("audio_plane_stride", was[2])
        if rate is not None:
            # a refused value leaves the options as they were: nothing has been set yet
            was = self.get_option("audio_rate"), self.get_option("audio_channels")
            self.set_option("audio_rate", int(rate))
            try:
                self.set_option("audio_channels", int(channels))
                return self._audio_call(ptr, mem, n, win, nwin, pcm16, cuts, None, 1, last, entries)
            finally:
                self.set_option("audio_rate", was[0])
                self.set_option("audio_channels", was[1])
        want = 1 if pcm16 else 0
        before = self.get_option("audio_format")             # a caller of the C-ABI may keep the option at 1: the samples handed over HERE decide
        if before != want:
            self.set_option("audio_format", want)
        try:
            try:
                for c in cuts:
                    self.set_option("audio_cut", int(c))
                for e in entries:
                    self.set_option("audio_track_slot", int(e))
            except Exception:
                self.set_option("audio_cut", -1)
                if entries:
                    self.set_option("audio_track_slot", -1)
                raise
            if last:
                self.set_option("audio_end", 1)
            self._check(self._L.avd_audio_features(self._h, ptr, mem, n, int(win), out.ctypes.data, nwin))
        finally:
            if before != want:
                self.set_option("audio_format", before)
        return out

    @staticmethod
    def _audio_frames(wav, channels: int):
        """-> (the interleaved samples as one flat array, channels): [n, c] names its own channel count, a flat array is n * channels samples"""
        if wav.ndim == 2:
            channels = int(wav.shape[1])
            wav = (wav.contiguous() if _is_torch_tensor(wav) else np.ascontiguousarray(wav)).reshape(-1)
        elif wav.ndim != 1:
            raise ValueError("wav must be [n * channels] or [n, channels]")
        if channels < 1 or int(wav.shape[0]) % channels:
            raise ValueError("wav does not hold whole frames of %d channels" % channels)
        return wav, channels

    AUDIO_LAYOUTS = (1, 2, 6, 8)             # option "audio_layout": mono, stereo, 5.1, 7.1 -- the id is the channel count
    AUDIO_PLANAR = 0x100

    def _audio_layout_source(self, wav, rate, layout, planar: bool):
        """A track with a layout (option "audio_layout") -> (ptr, mem, frames, pcm16, option value, plane stride, keepalive).  Interleaved: [n, c]
        or flat, as _audio_frames takes it.  planar: [c, n], and a column slice of a wider array (dense rows, one row stride) goes through as it
        lies, the row stride being the plane stride; anything else is copied dense first.  Device tensors likewise."""
        layout = int(layout)
        if rate is None:
            raise ValueError("layout needs rate: a layout describes a track at its decoder's rate")
        if layout not in self.AUDIO_LAYOUTS:
            raise ValueError("layout must be one of %s (the channel count)" % (self.AUDIO_LAYOUTS,))
        pcm16 = self._is_pcm16(wav)
        if not planar:
            flat, channels = self._audio_frames(wav, layout)
            if channels != layout:
                raise ValueError("wav holds frames of %d channels, layout %d" % (channels, layout))
            ptr, mem, size, keep = self._audio_ptr(flat, pcm16)
            return ptr, mem, size // layout, pcm16, layout, 0, keep
        if wav.ndim == 1 and layout == 1:
            wav = wav.reshape(1, -1)
        if wav.ndim != 2 or int(wav.shape[0]) != layout:
            raise ValueError("planar wav must be [%d, n]" % layout)
        n = int(wav.shape[1])
        if _is_torch_tensor(wav):
            if str(wav.dtype) != ("torch.int16" if pcm16 else "torch.float32"):
                raise ValueError("wav must be float32 or int16")
            t = wav
            if n and (t.stride(1) != 1 or (layout > 1 and t.stride(0) < n)):
                t = t.contiguous()
            if t.is_cuda:
                self._after_torch_stream(t)
            stride = int(t.stride(0)) if layout > 1 and n else n
            return t.data_ptr(), (AVD_MEM_DEVICE if t.is_cuda else AVD_MEM_HOST), n, pcm16, layout | self.AUDIO_PLANAR, stride, t
        item = 2 if pcm16 else 4
        a = np.asarray(wav, dtype=np.int16 if pcm16 else np.float32)
        if n and (a.strides[1] != item or (layout > 1 and (a.strides[0] < n * item or a.strides[0] % item))):
            a = np.ascontiguousarray(a)
        stride = a.strides[0] // item if layout > 1 and n else n
        return a.ctypes.data, AVD_MEM_HOST, n, pcm16, layout | self.AUDIO_PLANAR, stride, a

    def _audio_layout_join(self, tracks, rate, layout, planar: bool, what: str):
        """Several tracks with one layout, joined along the frame axis for one call -> (_audio_layout_source of the joined buffer, frames per track)"""
        pcm = {self._is_pcm16(t) for t in tracks}
        if len(pcm) != 1:
            raise ValueError("%s: the tracks must be all float32 or all int16" % what)
        on_device = {bool(_is_torch_tensor(t) and t.is_cuda) for t in tracks}
        if len(on_device) != 1:
            raise ValueError("%s: the tracks must be all host arrays or all device tensors" % what)
        layout = int(layout)
        if planar:
            tracks = [t.reshape(1, -1) if t.ndim == 1 and layout == 1 else t for t in tracks]
            if any(t.ndim != 2 or int(t.shape[0]) != layout for t in tracks):
                raise ValueError("planar wav must be [%d, n]" % layout)
            lens, axis = [int(t.shape[1]) for t in tracks], 1
        else:
            framed = [self._audio_frames(t, layout) for t in tracks]
            if any(c != layout for _, c in framed):
                raise ValueError("%s: the tracks must hold frames of %d channels" % (what, layout))
            tracks = [t.reshape(-1, layout) for t, _ in framed]
            lens, axis = [int(t.shape[0]) for t in tracks], 0
        if on_device.pop():
            import torch
            whole = torch.cat(list(tracks), dim=axis)
        else:
            whole = np.concatenate([np.asarray(t.numpy() if _is_torch_tensor(t) else t) for t in tracks], axis=axis)
        return self._audio_layout_source(whole, rate, layout, planar), lens

    AUDIO_SLOTS = 8

    @classmethod
    def audio_ratio(cls, rate):
        """-> (U, D, T) of the conversion rule (include/avd.h); rate None or 0 -- a track that is not converted -- is (1, 1, 0)"""
        if not rate:
            return 1, 1, 0
        g = math.gcd(int(rate), cls.AUDIO_OUT_RATE)
        U, D = cls.AUDIO_OUT_RATE // g, int(rate) // g
        if int(rate) == cls.AUDIO_OUT_RATE:
            return U, D, 0
        return U, D, 2 * math.ceil(16 / min(1.0, 0.97 * U / D))

    @classmethod
    def audio_outputs_after(cls, frames: int, rate, last: bool = False) -> int:
        """M of the audio slots' rule: the outputs that exist once a slot has absorbed ``frames`` frames -- ceil(max(0, N - T/2) U / D), and
        ceil(N U / D) after the last call"""
        U, D, T = cls.audio_ratio(rate)
        usable = int(frames) if last else max(0, int(frames) - T // 2)
        return -(-usable * U // D)

    def _audio_slot_features(self, wav, win: int, rate, channels: int, slot: int, last: bool, layout=None, planar: bool = False) -> np.ndarray:
        """audio_features with a slot: option "audio_slot" set for the call and restored, also after an exception"""
        code = stride = 0
        if layout is not None:
            ptr, mem, n, pcm16, code, stride, keep = self._audio_layout_source(wav, rate, layout, planar)
        else:
            pcm16 = self._is_pcm16(wav)
            if rate is not None:
                wav, channels = self._audio_frames(wav, channels)
            else:
                channels = 1
            ptr, mem, size, keep = self._audio_ptr(wav, pcm16)
            n = size // channels
        was = self.get_option("audio_slot")
        self.set_option("audio_slot", int(slot))          # a refused value leaves the option as it was
        try:
            # the record array, from the rule: W_after - W_before.  A slot past 2^31 - 1 frames reads back saturated; then an upper bound serves
            # (a written record has length >= 1, the array starts as zeros)
            frames, held = self.get_option("audio_slot_frames"), self.get_option("audio_slot_held")
            exact = frames < 0x7fffffff and 1 <= win <= 8192 and (rate is None or rate in self.AUDIO_RATES)
            if exact:
                fresh = self.audio_outputs_after(frames + n, rate, last) - self.audio_outputs_after(frames, rate)
                nwin = -(-(held + fresh) // win) if last else (held + fresh) // win
            elif 1 <= win <= 8192 and (rate is None or rate in self.AUDIO_RATES):
                U, D, T = self.audio_ratio(rate)
                nwin = (held + -(-(n + T) * U // D) + 1) // win + 1
            else:
                nwin = 0                                   # the library refuses (AvdError)
            rec = self._audio_call(ptr, mem, n, win, nwin, pcm16, (), rate, channels, last, (), code, stride)
            return rec if exact else rec[:int(np.count_nonzero(rec["length"]))]
        finally:
            self.set_option("audio_slot", was)

    def audio_features(self, wav, win: int, rate=None, channels: int = 1, slot: int = 0, last: bool = False, layout=None, planar: bool = False) -> np.ndarray:
        """wav: mono samples, float32 or 16-bit PCM as decoded (int16: sample s counts as float32(s) * 2^-15, converted on the device), numpy or
        torch-ROCm tensor -> structured array (AUDIO_WINDOW_DTYPE) per window.

        rate (one of AUDIO_RATES): wav is a track as its decoder produced it -- frames at ``rate``, [n] / [n, 1] mono or [n, 2] / flat with
        channels = 2 interleaved stereo -- and is downmixed, resampled to 16 kHz and narrowed to 16 bit on the device first (options "audio_rate" /
        "audio_channels", set for this call and restored); win and the records refer to the 16 kHz output.

        slot (1 ... AUDIO_SLOTS): the call CONTINUES the track of that audio slot (option "audio_slot", set for this call and restored, also after
        an exception) and returns the records of the windows this call completes -- possibly none; last=True marks the track's final call
        (option "audio_end"), which hands out the short last window and empties the slot.  wav may be empty.  The concatenated results of a
        track's calls are byte for byte the result of one slot-0 call on the joined samples.

        layout (one of AUDIO_LAYOUTS: 1 mono, 2 stereo, 6 5.1, 8 7.1 in FFmpeg's native channel order; needs rate): the track goes to the device as
        its decoder handed it over and is downmixed there by the layout's weights (options "audio_layout" / "audio_plane_stride", set for this call
        and restored; ``channels`` is not read).  wav is [n, layout] or flat interleaved; with planar=True it is [layout, n], one plane per channel,
        and a column slice of a wider array (ring[:, a:b]) goes through as it lies.  Without layout nothing of this is touched."""
        if slot:
            return self._audio_slot_features(wav, int(win), rate, channels, slot, bool(last), layout, bool(planar))
        if layout is not None:
            ptr, mem, n, pcm16, code, stride, keep = self._audio_layout_source(wav, rate, layout, planar)
            n_out = self.audio_converted_length(n, rate) if rate in self.AUDIO_RATES else 0          # another rate: the library refuses (AvdError)
            nwin = (n_out + win - 1) // win if n_out and win > 0 else 0
            return self._audio_call(ptr, mem, n, win, nwin, pcm16, (), rate, layout, False, (), code, stride)
        pcm16 = self._is_pcm16(wav)
        if rate is None:
            ptr, mem, n, keep = self._audio_ptr(wav, pcm16)
            nwin = (n + win - 1) // win if n and win > 0 else 0          # win < 1 or > 8192: the library refuses (AvdError)
            return self._audio_call(ptr, mem, n, win, nwin, pcm16)
        wav, channels = self._audio_frames(wav, channels)
        ptr, mem, size, keep = self._audio_ptr(wav, pcm16)
        n = size // channels
        n_out = self.audio_converted_length(n, rate) if rate in self.AUDIO_RATES else 0          # another rate: the library refuses (AvdError)
        nwin = (n_out + win - 1) // win if n_out and win > 0 else 0
        return self._audio_call(ptr, mem, n, win, nwin, pcm16, (), rate, channels)

    AUDIO_TRACKS_PER_CALL = 64

    def audio_features_many(self, tracks, win: int, rate=None, channels: int = 1, layout=None, planar: bool = False) -> list:
        """Several mono tracks in as few calls as possible (option "audio_cut": up to 64 tracks share one call and fill the chip together).
        tracks: all float32 or all int16, all host arrays (numpy, host tensors) or all device tensors.  Host tracks are concatenated once, device
        tracks go through one torch.cat.  -> one record array per track, in order: byte for byte what audio_features gives for that track alone.

        rate: every track is frames at that rate with the same channel count (see audio_features); the cuts are frame positions, and each track is
        converted from its own start.

        layout / planar: as for audio_features, the same for every track; planar tracks are [layout, n_i] and are joined along the frame axis."""
        tracks = list(tracks)
        if not tracks:
            return []
        if layout is not None:
            (ptr, mem, _, pcm16, code, stride, keep), lens = self._audio_layout_join(tracks, rate, layout, bool(planar), "audio_features_many")
            win = int(win)
            per = win if 1 <= win <= 8192 else 0
            analysed = [self.audio_converted_length(n, rate) if rate in self.AUDIO_RATES else 0 for n in lens]
            size = (2 if pcm16 else 4) * (1 if planar else int(layout))        # bytes from a frame to the next, in a plane or interleaved
            results = [None] * len(tracks)
            live = [i for i, n in enumerate(lens) if n > 0]
            starts = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            for g in range(0, len(live), self.AUDIO_TRACKS_PER_CALL):
                group = live[g:g + self.AUDIO_TRACKS_PER_CALL]
                first, end = int(starts[group[0]]), int(starts[group[-1] + 1])
                counts = [(analysed[i] + per - 1) // per if per else 0 for i in group]
                cuts = [int(starts[i]) - first for i in group[1:]]
                rec = self._audio_call(ptr + first * size, mem, end - first, win, sum(counts), pcm16, cuts, rate, int(layout), False, (), code, stride)
                at = 0
                for i, c in zip(group, counts):
                    results[i] = rec[at:at + c]
                    at += c
            for i, n in enumerate(lens):
                if n == 0:
                    results[i] = np.zeros(0, AUDIO_WINDOW_DTYPE)
            return results
        if rate is not None:
            framed = [self._audio_frames(t, channels) for t in tracks]
            if len({c for _, c in framed}) != 1:
                raise ValueError("audio_features_many: the tracks must have one channel count")
            tracks, channels = [t for t, _ in framed], framed[0][1]
        else:
            channels = 1
        pcm = {self._is_pcm16(t) for t in tracks}
        if len(pcm) != 1:
            raise ValueError("audio_features_many: the tracks must be all float32 or all int16")
        pcm16 = pcm.pop()
        on_device = {bool(_is_torch_tensor(t) and t.is_cuda) for t in tracks}
        if len(on_device) != 1:
            raise ValueError("audio_features_many: the tracks must be all host arrays or all device tensors")
        if any(t.ndim != 1 for t in tracks):
            raise ValueError("wav must be float32[n] or int16[n]")
        win = int(win)
        per = win if 1 <= win <= 8192 else 0                         # win < 1 or > 8192: the library refuses (AvdError)
        lens = [int(t.shape[0]) // channels for t in tracks]          # frames
        if rate is None:
            analysed = lens                                           # samples the analyzer windows, per track
        elif rate in self.AUDIO_RATES:
            analysed = [self.audio_converted_length(n, rate) for n in lens]
        else:
            analysed = [0] * len(lens)                                # another rate: the library refuses (AvdError)
        if on_device.pop():
            import torch
            whole = torch.cat([t if pcm16 else t.to(torch.float32) for t in tracks])
        else:
            dt = np.int16 if pcm16 else np.float32
            whole = np.concatenate([np.asarray(t.numpy() if _is_torch_tensor(t) else t, dtype=dt) for t in tracks])
        ptr, mem, _, keep = self._audio_ptr(whole, pcm16)
        size = (2 if pcm16 else 4) * channels
        results = [None] * len(tracks)
        # an empty track has no window and cannot be cut off (cuts ascend strictly): it gets its empty result here and stays out of the calls
        live = [i for i, n in enumerate(lens) if n > 0]
        starts = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        for g in range(0, len(live), self.AUDIO_TRACKS_PER_CALL):
            group = live[g:g + self.AUDIO_TRACKS_PER_CALL]
            first, end = int(starts[group[0]]), int(starts[group[-1] + 1])
            counts = [(analysed[i] + per - 1) // per if per else 0 for i in group]
            cuts = [int(starts[i]) - first for i in group[1:]]
            rec = self._audio_call(ptr + first * size, mem, end - first, win, sum(counts), pcm16, cuts, rate, channels)
            at = 0
            for i, c in zip(group, counts):
                results[i] = rec[at:at + c]
                at += c
        for i, n in enumerate(lens):
            if n == 0:
                results[i] = np.zeros(0, AUDIO_WINDOW_DTYPE)
        return results

    AUDIO_TRACK_END = 0x10

    def audio_features_mapped(self, chunks, slots, lasts, win: int, rate=None, channels: int = 1, layout=None, planar: bool = False) -> list:
        """Several tracks in ONE call, each a whole track or the continuation of an audio slot (option "audio_track_slot", set for this call; it and
        the cuts are gone after it, also after an exception).  chunks[i] is what audio_features takes for one track -- all float32 or all int16, all
        host arrays or all device tensors, at least one frame each; slots[i] = 0 says it is a whole track, 1 ... AUDIO_SLOTS that it continues that
        slot (each slot once); lasts[i] that it carries the slot's last samples.  Host chunks are concatenated once, device chunks go through one
        torch.cat.  -> one record array per track, in order: for a slot the windows this call completes (possibly none), the concatenated results
        of a track's calls being byte for byte the result of one slot-0 call on the joined samples.  The gather, converter, analyzer and save each
        run once per call, however many tracks it has.

        layout / planar: as for audio_features, the same for every chunk; planar chunks are [layout, n_i] and are joined along the frame axis."""
        chunks, slots, lasts = list(chunks), [int(s) for s in slots], [bool(l) for l in lasts]
        if not chunks or not (len(chunks) == len(slots) == len(lasts)):
            raise ValueError("audio_features_mapped: one slot and one end mark per chunk, at least one chunk")
        if len(chunks) > self.AUDIO_TRACKS_PER_CALL:
            raise ValueError("audio_features_mapped: at most %d tracks per call" % self.AUDIO_TRACKS_PER_CALL)
        joined = None
        if layout is not None:
            joined, lens = self._audio_layout_join(chunks, rate, layout, bool(planar), "audio_features_mapped")
            pcm16, channels = joined[3], int(layout)
        elif rate is not None:
            framed = [self._audio_frames(t, channels) for t in chunks]
            if len({c for _, c in framed}) != 1:
                raise ValueError("audio_features_mapped: the tracks must have one channel count")
            chunks, channels = [t for t, _ in framed], framed[0][1]
        else:
            channels = 1
        if joined is None:
            pcm = {self._is_pcm16(t) for t in chunks}
            if len(pcm) != 1:
                raise ValueError("audio_features_mapped: the tracks must be all float32 or all int16")
            pcm16 = pcm.pop()
            on_device = {bool(_is_torch_tensor(t) and t.is_cuda) for t in chunks}
            if len(on_device) != 1:
                raise ValueError("audio_features_mapped: the tracks must be all host arrays or all device tensors")
            if any(t.ndim != 1 for t in chunks):
                raise ValueError("wav must be float32[n] or int16[n]")
            lens = [int(t.shape[0]) // channels for t in chunks]          # frames
        if min(lens) < 1:
            raise ValueError("audio_features_mapped: every track of the call needs a frame (flush an empty stream with audio_features(..., slot=k, last=True))")
        win = int(win)
        known = 1 <= win <= 8192 and (rate is None or rate in self.AUDIO_RATES)       # otherwise the library refuses (AvdError)
        # the record arrays, from the rule (what _audio_slot_features does for one slot); the read-only options want their slot selected, which the
        # list excludes -- so this comes before the list is set
        counts = []
        was = self.get_option("audio_slot")
        try:
            for n, slot, last in zip(lens, slots, lasts):
                if not known:
                    counts.append(0)
                elif slot == 0:
                    counts.append(-(-self.audio_outputs_after(n, rate, True) // win))
                else:
                    self.set_option("audio_slot", slot)
                    frames, held = self.get_option("audio_slot_frames"), self.get_option("audio_slot_held")
                    if frames < 0x7fffffff:
                        fresh = self.audio_outputs_after(frames + n, rate, last) - self.audio_outputs_after(frames, rate)
                        counts.append(-(-(held + fresh) // win) if last else (held + fresh) // win)
                    else:
                        raise ValueError("audio_features_mapped: slot %d has absorbed more than 2^31 - 1 frames; continue it with audio_features(slot=)" % slot)
            self.set_option("audio_slot", 0)
            code = stride = 0
            if joined is not None:
                ptr, mem, _, _, code, stride, keep = joined
            elif on_device.pop():
                import torch
                whole = torch.cat([t if pcm16 else t.to(torch.float32) for t in chunks])
                ptr, mem, _, keep = self._audio_ptr(whole, pcm16)
            else:
                dt = np.int16 if pcm16 else np.float32
                whole = np.concatenate([np.asarray(t.numpy() if _is_torch_tensor(t) else t, dtype=dt) for t in chunks])
                ptr, mem, _, keep = self._audio_ptr(whole, pcm16)
            cuts = [int(c) for c in np.cumsum(lens)[:-1]]
            entries = [s | (self.AUDIO_TRACK_END if (l and s) else 0) for s, l in zip(slots, lasts)]
            rec = self._audio_call(ptr, mem, sum(lens), win, sum(counts), pcm16, cuts, rate, channels, False, entries, code, stride)
        finally:
            self.set_option("audio_slot", was)               # also after an exception (no list is held then: the call has taken it, or a failure cleared it)
        out, at = [], 0
        for c in counts:
            out.append(rec[at:at + c])
            at += c
        return out

    def audio_map_call(self):
        """(tracks, continued tracks, gather launches, converter launches, analyzer passes, save launches) of the last audio_features_mapped call;
        avd_debug_fetch "audio_map_call"."""
        return tuple(int(v) for v in self.debug_fetch("audio_map_call", (6,), np.int32))

    def audio_layout(self) -> np.ndarray:
        """int32[12] of the last call that converted: layout id (0: it went by "audio_channels"), planar 0 / 1, channels, the plane stride in
        effect, the eight Q15 downmix weights; avd_debug_fetch "audio_layout"."""
        return self.debug_fetch("audio_layout", (12,), np.int32)

    def audio_tracks(self) -> np.ndarray:
        """int32[tracks, 3] of the last audio_features / audio_features_many call that ran: per track its first window, its windows and the length
        of its last window; avd_debug_fetch "audio_tracks"."""
        out = np.zeros((self.AUDIO_TRACKS_PER_CALL, 3), np.int32)
        got = self._L.avd_debug_fetch(self._h, b"audio_tracks", out.ctypes.data, out.nbytes)
        if got < 0:
            self._check(int(got))
        return out[:got // 12].copy()

    def audio_resample_plan(self):
        """(rate, channels, U, D, T, outputs per tile, input frames, output samples) of the last audio_features call, which converted its input
        (rate given); avd_debug_fetch "audio_rs_plan"."""
        return tuple(int(v) for v in self.debug_fetch("audio_rs_plan", (8,), np.int32))

    def audio_resample_taps(self) -> np.ndarray:
        """int32[U, T]: the filter bank that call ran with (empty at rate 16000, which has none); avd_debug_fetch "audio_rs_taps"."""
        _, _, U, _, T, _, _, _ = self.audio_resample_plan()
        return self.debug_fetch("audio_rs_taps", (U, T), np.int32) if U * T else np.zeros((U, 0), np.int32)

    def audio_resample_tracks(self) -> np.ndarray:
        """int32[tracks, 2]: per track of that call its first output sample in the converted buffer and its output samples; avd_debug_fetch
        "audio_rs_tracks"."""
        out = np.zeros((self.AUDIO_TRACKS_PER_CALL, 2), np.int32)
        got = self._L.avd_debug_fetch(self._h, b"audio_rs_tracks", out.ctypes.data, out.nbytes)
        if got < 0:
            self._check(int(got))
        return out[:got // 8].copy()

    def audio_pcm(self) -> np.ndarray:
        """int16[output samples]: the converted tracks of that call, side by side -- what the analyzer ran over; avd_debug_fetch "audio_pcm"."""
        n = self.audio_resample_plan()[7]                   # a slot call: its new outputs only, possibly none
        return self.debug_fetch("audio_pcm", (n,), np.int16) if n else np.zeros(0, np.int16)

    def audio_plan(self):
        """(nwin, win, last, nfull) of the last audio_features call: windows, window length, length of the last window, windows that
        took the 80 x 100 transform (the rest took the direct sum); avd_debug_fetch "audio_plan"."""
        return tuple(int(v) for v in self.debug_fetch("audio_plan", (4,), np.int32))

    def audio_xw(self) -> np.ndarray:
        """float64[nwin, win]: the windowed samples of the last audio_features call (a short last window fills only its first
        ``last`` entries); avd_debug_fetch "audio_xw"."""
        nwin, win, _, _ = self.audio_plan()
        return self.debug_fetch("audio_xw", (nwin, win), np.float64)

    def audio_mag(self) -> np.ndarray:
        """float64[nwin, win // 2 + 1]: |rfft| + 1e-9 per window of the last audio_features call (a short last window: its first
        ``last // 2 + 1`` entries); avd_debug_fetch "audio_mag"."""
        nwin, win, _, _ = self.audio_plan()
        return self.debug_fetch("audio_mag", (nwin, win // 2 + 1), np.float64)

    # -- record exchange across ranks (RCCL, bound at run time) --------------------------------------------------
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        rc = load().avd_comm_unique_id(buf)
        if rc != 0:
            raise AvdError(f"avd_comm_unique_id failed with status {rc} (is librccl.so available?)")
        return buf.raw

    def comm_init(self, rank: int, world: int, unique_id: bytes):
        assert len(unique_id) == 128
        self._check(self._L.avd_comm_init(self._h, int(rank), int(world), C.create_string_buffer(unique_id, 128)))
        self._comm_world = int(world)

    def allgather_records(self, local: np.ndarray) -> np.ndarray:
        local = np.ascontiguousarray(local)
        assert local.dtype == RECORD_DTYPE
        out = np.zeros(len(local) * getattr(self, "_comm_world", 1), RECORD_DTYPE)
        self._check(self._L.avd_allgather_records(self._h, local.ctypes.data, len(local), out.ctypes.data))
        return out

    def allgather_last_records(self, count: int) -> np.ndarray:
        """Gather the first ``count`` records of this context's last analysis call from every rank, straight from HBM
        (enqueued behind the analysis on the context's stream; drains an outstanding asynchronous call)."""
        out = np.zeros(count * getattr(self, "_comm_world", 1), RECORD_DTYPE)
        self._check(self._L.avd_allgather_last_records(self._h, count, out.ctypes.data))
        return out

    def analyze_frames_async(self, frames, rec: np.ndarray):
        return self._analyze("avd_analyze_frames_async", self._bgr(frames), rec)          # the buffer the kernels read: the caller holds it until synchronize()

    def synchronize(self):
        self._check(self._L.avd_synchronize(self._h))
        self._list_keep = None

    # -- a batch of clips in one call (include/avd.h: avd_analyze_batch) -----------------------------------------
    def _clip_array(self, clips):
        """clips: sequence of BGR frame stacks uint8[N,H,W,3] or NV12 plane pairs (y, uv); numpy or torch, any mix of
        geometries -> (AvdClip array, frame counts, keepalive)"""
        arr = (AvdClip * len(clips))()
        keep, counts = [], []
        for i, c in enumerate(clips):
            if isinstance(c, tuple):
                yp, cp, mem, n, h, w, yr, cr, yf, cf, k = self._nv12_ptrs(*c)
                arr[i] = AvdClip(yp, cp, mem, n, h, w, yr, yf, cr, cf)
            else:
                ptr, mem, n, h, w, rs, fs, k = self._frames_ptr(c)
                arr[i] = AvdClip(ptr, None, mem, n, h, w, rs, fs, 0, 0)
            keep.append(k)
            counts.append(n)
        return arr, counts, keep

    def analyze_batch(self, clips):
        """-> list of record arrays, one per clip (identical to analyze_frames / analyze_frames_nv12 per clip)."""
        arr, counts, keep = self._clip_array(clips)
        rec = self._records_call("avd_analyze_batch", (arr, len(clips)), sum(counts))
        return list(np.split(rec, np.cumsum(counts)[:-1])) if counts else []

    def analyze_batch_async(self, clips, rec: np.ndarray):
        """Enqueue only; rec (RECORD_DTYPE, sum of the clips' frames) is filled by synchronize().  Returns what the caller
        must keep alive until then."""
        arr, counts, keep = self._clip_array(clips)
        self._records_call("avd_analyze_batch_async", (arr, len(clips)), sum(counts), rec)
        return keep, counts

    def wait_stream(self, stream_handle: int = 0):
        """Order this context's stream behind everything already enqueued on another HIP stream (raw handle)."""
        self._check(self._L.avd_wait_stream(self._h, C.c_void_p(stream_handle)))

    def release_workspace(self):
        self._check(self._L.avd_release_workspace(self._h))

    def timer_start(self):
        self._check(self._L.avd_timer_start(self._h))

    def timer_stop(self) -> float:
        ms = C.c_float()
        self._check(self._L.avd_timer_stop(self._h, C.byref(ms)))
        return float(ms.value)

    def set_option(self, name: str, value: int):
        """Tuning / test switches, e.g. ``set_option("fb_fused", 0)`` selects the two-kernel Farneback path."""
        self._check(self._L.avd_set_option(self._h, name.encode(), int(value)))

    def get_option(self, name: str) -> int:
        """Current value of an option (environment defaults included), or a read-only counter such as ``rerun_pairs``."""
        v = C.c_int()
        self._check(self._L.avd_get_option(self._h, name.encode(), C.byref(v)))
        return int(v.value)

    # -- stream slots (include/avd.h, options "stream_slot" / "stream_reset" / "stream_frames"): calls that continue one clip ----------------
    def stream_slot(self, slot: int = 0):
        """Select slot 1 ... 8: every analyze_* call of ONE clip then continues the clip whose last frame the slot holds (its first record is
        that of the pair across the call boundary) and leaves its own last frame there.  0 (default): every call starts a new clip."""
        self.set_option("stream_slot", slot)

    def stream_reset(self, slot: int = 0):
        """Empty slot 1 ... 8, or with 0 all of them: the next call on it starts a clip."""
        self.set_option("stream_reset", slot)

    def stream_frames(self) -> int:
        """Frames the selected slot has absorbed since it was last emptied (0: it is empty, or no slot is selected)."""
        return self.get_option("stream_frames")

    # -- several clips of ONE call continue a slot each (include/avd.h, option "stream_map") -------------------------------------------------
    def stream_map(self, mapping=None):
        """mapping: {clip position 0 ... 63: slot 1 ... 8} -- the clip at that position of every following analyze_* call continues that slot,
        every other clip starts a new one.  The map is replaced by `mapping`; None or {} clears it.  A refused entry leaves the map empty."""
        self.set_option("stream_map", -1)
        try:
            for position, slot in sorted((mapping or {}).items()):
                position, slot = int(position), int(slot)
                if not 0 <= position <= 63 or not 1 <= slot <= 8:
                    raise ValueError(f"stream_map: position 0 ... 63 -> slot 1 ... 8, got {position} -> {slot}")
                self.set_option("stream_map", (position << 4) | slot)
        except Exception:
            self.set_option("stream_map", -1)
            raise

    def stream_state(self) -> np.ndarray:
        """int32[8][2]: per slot the frames it has absorbed since it was last emptied and the clip position mapped to it (-1: none);
        avd_debug_fetch "stream_state"."""
        return self.debug_fetch("stream_state", (8, 2), np.int32)

    def stream_call(self) -> np.ndarray:
        """int32[4] of the last analyze_* call: clips that continued a filled slot, restore launches, save launches, frames in the per-frame
        buffers (restored frames included); avd_debug_fetch "stream_call"."""
        return self.debug_fetch("stream_call", (4,), np.int32)

    # -- option "ingest_group" (include/avd.h): the clips of a call that share a key share one ingest and one hash launch ---------------------
    def ingest_call(self) -> np.ndarray:
        """int32[4] of the last analyze_* call: ingest launches, hash launches, groups of more than one clip, frames ingested by grouped
        launches; avd_debug_fetch "ingest_call"."""
        return self.debug_fetch("ingest_call", (4,), np.int32)

    def ingest_groups(self) -> np.ndarray:
        """int32[launches][4] of that call, in launch order: first clip position, clips, frames, kernel id (as in ingest_plan);
        avd_debug_fetch "ingest_groups"."""
        launches = int(self.ingest_call()[0])
        return self.debug_fetch("ingest_groups", (launches, 4), np.int32) if launches else np.zeros((0, 4), np.int32)

    # -- option "cv2_model" (include/avd.h): the library follows the oracle's model switches; set with set_option("cv2_model", mask) -----------
    def fb_model(self) -> np.ndarray:
        """int32[4] of the last call that ran the Farneback stage: the cv2_model it ran under, the scales it ran (4 or 3), the fb_fold_up mask
        in effect, fb_fold_blur in effect; avd_debug_fetch "fb_model"."""
        return self.debug_fetch("fb_model", (4,), np.int32)

    def set_profiling(self, on: bool):
        self._check(self._L.avd_set_profiling(self._h, int(bool(on))))

    def stage_ms(self):
        out = []
        for i in range(6):
            ms = C.c_float()
            self._check(self._L.avd_stage_ms(self._h, i, C.byref(ms)))
            out.append(float(ms.value))
        return out

    KERNEL_IDS = ("preprocess", "hash", "pyramid", "polyexp", "level40", "flow_up80", "level80", "flow_up160", "level160",
                  "flow_up320", "level320", "rerun", "stats", "records", "other")      # enum avd_kernel_id

    def kernel_ms(self) -> dict:
        """Per-kernel device time (ms) of the last drained call with profiling on (avd_kernel_ms)."""
        out = {}
        for i, name in enumerate(self.KERNEL_IDS):
            ms = C.c_float()
            self._check(self._L.avd_kernel_ms(self._h, i, C.byref(ms)))
            out[name] = float(ms.value)
        return out

    def debug_fetch(self, name: str, shape, dtype) -> np.ndarray:
        out = np.empty(shape, dtype)
        got = self._L.avd_debug_fetch(self._h, name.encode(), out.ctypes.data, out.nbytes)
        if got < 0:
            self._check(int(got))
        if got != out.nbytes:
            raise AvdError(f"debug buffer {name}: expected {out.nbytes} bytes, got {got}")
        return out
