"""Runtime-probed frame sources for ``app.analyzers.video.analyze(path, meta)``.

Container demux/decode (reference app/analyzers/video.py:11,28,32 -> cv2.VideoCapture /
libavcodec) is outside the parity boundary of this build: it is
third-party host plumbing, and none of cv2 / PyAV / ffmpeg exists in the build image.  A
source only has to yield what ``cap.retrieve()`` yields -- BGR uint8[H,W,3] -- for the frames
whose index is a multiple of ``step`` (every frame is still *grabbed*, i.e. decoded), plus the
capture properties the reference falls back to when ffprobe metadata is missing
(video.py:14-17).  Probed in this order:

  1. ``*.npy``  raw decoded stack uint8[T,H,W,3] (memory-mapped) -- used by tests / tools;
  2. ``*.y4m``  YUV4MPEG2, 8-bit 4:2:0 or 4:2:2 (a ``C422`` file goes, as the file's own planes, through the 4:2:2 ingest; what ``ffmpeg -i in.mp4 out.y4m`` writes, i.e. a decoder's pictures BEFORE the colour
     conversion): memory-mapped, handed over as NV12 surfaces to ``avd_analyze_frames_nv12`` -- the YUV->BGR step of
     ``cap.retrieve()`` happens in the HIP kernel, no BGR frame ever exists.  With
     ``planar=True`` (or ``AVD_Y4M_SURFACE=i420``) the file's own planar pictures go to ``avd_analyze_frames_i420`` as views of
     the map, without the host-side interleave;
  3. ``cv2.VideoCapture`` if OpenCV is importable (identical decode to the reference);
  4. ``ffmpeg``/``ffprobe`` CLIs if on PATH (rawvideo bgr24 pipe).
If nothing can open the file the analyzer returns the reference's "capture not opened"
result (video.py:12-13).
"""
from __future__ import annotations

import json
import os
import shutil
import subprocess
from typing import Iterator, Optional

import numpy as np


class FrameSource:
    # what sampled() yields: "bgr" = uint8[H,W,3]; "nv12" = (y uint8[H,W], uv uint8[H/2,W] interleaved U,V); "i420" = (y uint8[H,W], u uint8[H/2,W/2], v likewise);
    # "i422" = (y uint8[H,W], u uint8[H,W/2], v likewise), H even or odd;
    # "rgb24" = uint8[H,W,3] R,G,B; "bgra32" / "rgba32" = uint8[H,W,4], fourth byte ignored; "rgbp" = uint8[3,H,W] R,G,B planes (channels first)
    surface: str = "bgr"
    fps: float = 0.0
    width: int = 0
    height: int = 0
    frame_count: int = 0
    # quarter turns clockwise from the pictures sampled() yields (the STORED ones) to the displayed picture; width / height are the displayed
    # picture's, as cv2's capture properties are (orientation-auto)
    rotate: int = 0
    # the 4:2:0 / 4:2:2 pictures sampled() yields are full range (0 .. 255: ffmpeg's yuvj420p); means nothing for a source that yields BGR
    full_range: bool = False

    def sampled(self, step: int) -> Iterator[np.ndarray]:
        raise NotImplementedError

    def close(self) -> None:
        pass


class NpySource(FrameSource):
    def __init__(self, path: str):
        arr = np.load(path, mmap_mode="r")
        if arr.ndim != 4 or arr.shape[-1] != 3 or arr.dtype != np.uint8:
            raise ValueError("expected uint8[T,H,W,3]")
        self._arr = arr
        self.frame_count, self.height, self.width = int(arr.shape[0]), int(arr.shape[1]), int(arr.shape[2])

    def sampled(self, step):
        for i in range(0, self.frame_count, step):
            yield np.ascontiguousarray(self._arr[i])


class Y4mSource(FrameSource):
    """YUV4MPEG2 file with 8-bit 4:2:0 pictures (C420, C420jpeg, C420mpeg2, C420paleo -- chroma siting does not enter
    libswscale's unscaled yuv420p -> bgr24 conversion, which takes the nearest chroma sample).  Frames are read through a
    memory map; ``sampled`` yields NV12 surfaces (the U and V planes interleaved on the host: 0.5 byte per pixel), or with
    ``planar=True`` the file's own I420 planes as three views of the map (no copy, no interleave).
    A header token ``XAVD_ROTATE=<0|90|180|270>`` (YUV4MPEG2 ``X`` tokens are application comments that other readers ignore) carries a
    container's display rotation, clockwise: ``rotate`` is its quarter turns, ``width`` / ``height`` are the DISPLAYED picture's, the planes
    yielded are the stored ones.  ``XCOLORRANGE=FULL`` (what ffmpeg's y4m muxer writes for yuvj420p) sets ``full_range``; ``XCOLORRANGE=LIMITED``
    and no token mean limited range.
    ``C422`` (8-bit 4:2:2: what ffmpeg writes for yuv422p / yuvj422p, i.e. for MJPEG, webcam and capture-card sources): the chroma planes
    have H rows of W/2 samples, a frame is 2WH bytes, H may be odd; ``sampled`` always yields the file's own three planes as views of the
    map and ``surface`` is "i422", whatever ``planar`` says."""
    surface = "nv12"

    def __init__(self, path: str, planar: bool = False):
        self.surface = "i420" if planar else "nv12"
        with open(path, "rb") as f:
            header = f.readline(4096)
        if not header.startswith(b"YUV4MPEG2 ") or not header.endswith(b"\n"):
            raise ValueError("not a YUV4MPEG2 stream")
        self._data_off = len(header)
        w = h = 0
        num, den, chroma = 0, 1, "420"
        for tok in header.split()[1:]:
            tag, val = tok[:1], tok[1:].decode("ascii", "replace")
            if tag == b"W":
                w = int(val)
            elif tag == b"H":
                h = int(val)
            elif tag == b"F":
                a, _, b = val.partition(":")
                num, den = int(a), int(b or 1)
            elif tag == b"C":
                chroma = val
            elif tag == b"X" and val.startswith("AVD_ROTATE="):
                deg = val[len("AVD_ROTATE="):]
                if deg not in ("0", "90", "180", "270"):
                    raise ValueError("XAVD_ROTATE must be 0, 90, 180 or 270")
                self.rotate = int(deg) // 90
            elif tag == b"X" and val.startswith("COLORRANGE="):
                rng = val[len("COLORRANGE="):]
                if rng not in ("FULL", "LIMITED"):
                    raise ValueError("XCOLORRANGE must be FULL or LIMITED")
                self.full_range = rng == "FULL"
        c422 = chroma == "422"
        if w <= 0 or h <= 0 or w & 1 or (h & 1 and not c422):        # 4:2:2 subsamples nothing vertically: its height may be odd
            raise ValueError("bad or odd picture size")
        if not c422 and (not chroma.startswith("420") or "p1" in chroma):      # 420p10 / p12 / p16, 422p10 ...: more than 8 bits
            raise ValueError("only 8-bit 4:2:0 and 4:2:2 are supported")
        if c422:
            self.surface = "i422"
        self._w, self._h = w, h                                      # the stored picture
        self.width, self.height = (h, w) if self.rotate & 1 else (w, h)
        self.fps = num / den if den else 0.0
        self._crows = h if c422 else h // 2
        self._luma, self._chroma = w * h, (w // 2) * self._crows
        self._frame_bytes = self._luma + 2 * self._chroma
        self._map = np.memmap(path, dtype=np.uint8, mode="r")
        # every picture is preceded by "FRAME" [parameters] "\n"; the marker length is constant in files written by ffmpeg,
        # but it is read per frame anyway
        self._offsets = []
        pos = self._data_off
        size = self._map.shape[0]
        while pos + 6 <= size:
            end = pos
            limit = min(size, pos + 256)
            while end < limit and self._map[end] != 0x0A:
                end += 1
            if end >= limit or bytes(self._map[pos:pos + 5]) != b"FRAME":
                break
            if end + 1 + self._frame_bytes > size:
                break
            self._offsets.append(end + 1)
            pos = end + 1 + self._frame_bytes
        self.frame_count = len(self._offsets)

    def sampled(self, step):
        h, w = self._h, self._w
        for i in range(0, self.frame_count, step):
            o = self._offsets[i]
            y = np.asarray(self._map[o:o + self._luma]).reshape(h, w)
            u = self._map[o + self._luma:o + self._luma + self._chroma].reshape(self._crows, w // 2)
            v = self._map[o + self._luma + self._chroma:o + self._frame_bytes].reshape(self._crows, w // 2)
            if self.surface in ("i420", "i422"):
                yield self._map[o:o + self._luma].reshape(h, w), u, v
                continue
            uv = np.empty((h // 2, w), np.uint8)
            uv[:, 0::2] = u
            uv[:, 1::2] = v
            yield y, uv

    def close(self):
        self._map = None


def write_y4m(path: str, y: np.ndarray, uv: np.ndarray, fps=(30, 1), rotate: int = 0, full_range: bool = False) -> None:
    """NV12 surfaces (y uint8[N,H,W], uv uint8[N,H/2,W] interleaved) -> a YUV4MPEG2 file (tests, tools).  rotate: display rotation in
    DEGREES clockwise, written as the XAVD_ROTATE token when non-zero (Y4mSource); full_range: the XCOLORRANGE=FULL token, written only
    when true.  A uv of H rows (NV16: uint8[N,H,W]) is written as C422."""
    n, h, w = y.shape
    tag = b"C422" if uv.shape[1] == h else b"C420jpeg"
    with open(path, "wb") as f:
        f.write(b"YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 %s%s%s\n" % (w, h, fps[0], fps[1], tag, b" XAVD_ROTATE=%d" % rotate if rotate else b"",
                                                              b" XCOLORRANGE=FULL" if full_range else b""))
        for i in range(n):
            f.write(b"FRAME\n")
            f.write(np.ascontiguousarray(y[i]).tobytes())
            f.write(np.ascontiguousarray(uv[i][:, 0::2]).tobytes())
            f.write(np.ascontiguousarray(uv[i][:, 1::2]).tobytes())


class Cv2Source(FrameSource):
    def __init__(self, path: str, cv2):
        self._cv2 = cv2
        self._cap = cv2.VideoCapture(path)
        if not self._cap.isOpened():
            raise ValueError("capture not opened")
        self.fps = float(self._cap.get(cv2.CAP_PROP_FPS) or 0.0)
        self.width = int(self._cap.get(cv2.CAP_PROP_FRAME_WIDTH) or 0)
        self.height = int(self._cap.get(cv2.CAP_PROP_FRAME_HEIGHT) or 0)
        self.frame_count = int(self._cap.get(cv2.CAP_PROP_FRAME_COUNT) or 0)

    def sampled(self, step):
        index = 0
        while self._cap.grab():
            if index % step == 0:
                ok, frame = self._cap.retrieve()
                if not ok:
                    break
                yield frame
            index += 1

    def close(self):
        self._cap.release()


class FfmpegSource(FrameSource):
    def __init__(self, path: str):
        info = json.loads(subprocess.check_output(
            ["ffprobe", "-v", "error", "-select_streams", "v:0", "-show_entries",
             "stream=width,height,r_frame_rate,nb_frames", "-of", "json", path], text=True, timeout=30))
        st = info["streams"][0]
        self.width, self.height = int(st["width"]), int(st["height"])
        num, den = (st.get("r_frame_rate") or "0/1").split("/")
        self.fps = float(num) / max(1.0, float(den))
        try:
            self.frame_count = int(st.get("nb_frames") or 0)
        except ValueError:
            self.frame_count = 0
        self._path = path
        self._proc = None

    def sampled(self, step):
        self._proc = subprocess.Popen(["ffmpeg", "-v", "error", "-i", self._path, "-f", "rawvideo",
                                       "-pix_fmt", "bgr24", "-"], stdout=subprocess.PIPE)
        nbytes = self.width * self.height * 3
        index = 0
        while True:
            buf = self._proc.stdout.read(nbytes)
            if len(buf) < nbytes:
                break
            if index % step == 0:
                yield np.frombuffer(buf, np.uint8).reshape(self.height, self.width, 3)
            index += 1

    def close(self):
        if self._proc is not None:
            self._proc.kill()
            self._proc.wait()


def open_source(path: str, planar: Optional[bool] = None) -> Optional[FrameSource]:
    """First source that can open ``path``; None if none can (== capture not opened).  ``planar`` selects what a ``.y4m`` file yields:
    True = its own I420 planes, False = NV12; None reads the environment variable AVD_Y4M_SURFACE (``i420`` = planar, anything else or
    unset = NV12)."""
    if planar is None:
        planar = os.getenv("AVD_Y4M_SURFACE", "") == "i420"
    if str(path).endswith(".npy"):
        try:
            return NpySource(path)
        except (OSError, ValueError):
            return None
    if str(path).endswith(".y4m"):
        try:
            return Y4mSource(path, planar=bool(planar))
        except (OSError, ValueError):
            return None
    try:
        import cv2  # type: ignore
    except ImportError:
        cv2 = None
    if cv2 is not None:
        try:
            return Cv2Source(path, cv2)
        except ValueError:
            return None
    if shutil.which("ffmpeg") and shutil.which("ffprobe"):
        try:
            return FfmpegSource(path)
        except (subprocess.SubprocessError, KeyError, IndexError, ValueError, OSError):
            return None
    return None
