"""Cameras and pixel observations: the envs ray-cast on the GPU (``ps_render``).

* :class:`Camera` and :data:`CAMERAS` - the six named piano cameras of
  ``robopianist/models/piano/piano.py:100-141``, restated as a table.
* :func:`render` - ``BatchedPianoEnv.render``: N envs through one camera into one torch tensor.
* :class:`Physics` - ``Environment.physics``: the reference's single-env spelling,
  ``physics.render(height, width, camera_id, depth, segmentation)`` -> numpy.
* :class:`PixelWrapper` - ``robopianist/wrappers/pixels.py`` over an ``Environment`` or a
  ``VectorizedPianoEnv``.
* :func:`write_png` - an image file with the standard library alone.

The scene, the conventions, the segmentation ids and the shading formula are stated in
include/pianosim.h (``ps_render``) and DESIGN.md section 16. No CPU fallback: rendering needs the
library and a GPU.
"""

from __future__ import annotations

import collections
import ctypes as C
import math
import struct
import zlib
from typing import Any, Dict, Optional, Sequence, Union

import numpy as np

from . import _lib

# ps_render flags and segmentation ids (include/pianosim.h)
RENDER_ACTIVATION = 1 << 0
RENDER_COLORIZE = 1 << 1
RENDER_COUNT_LIST = 1 << 16
SEG_KEY0, SEG_BASE, SEG_FLOOR = 64, 152, 153
AMBIENT, DIFFUSE = 0.3, 0.7
# PS_RENDER_COLOR_*: white key, black key, base, activated key, the five fingers (th ff mf rf lf),
# hand, floor, background
COLORS = np.array([(0.9, 0.9, 0.9), (0.1, 0.1, 0.1), (0.15, 0.15, 0.15), (0.2, 0.8, 0.2),
                   (0.8, 0.2, 0.8), (0.8, 0.2, 0.2), (0.2, 0.8, 0.8), (0.2, 0.2, 0.8), (0.8, 0.8, 0.2),
                   (0.6, 0.6, 0.6), (0.2, 0.3, 0.4), (0.05, 0.05, 0.1)])
COLOR_WHITE, COLOR_BLACK, COLOR_BASE, COLOR_ACTIVATION, COLOR_FINGER0, COLOR_HAND, COLOR_FLOOR, COLOR_BACKGROUND = \
    0, 1, 2, 3, 4, 9, 10, 11


class CameraDesc(C.Structure):  # ps_camera
    _fields_ = [("pos", C.c_double * 3), ("x", C.c_double * 3), ("y", C.c_double * 3), ("fovy_deg", C.c_double)]


class Camera:
    """A pinhole camera as MJCF writes one: ``pos``, ``xyaxes`` (image right, then image up; made
    orthonormal here, x first, as MuJoCo's compiler does) and the vertical field of view ``fovy``
    in degrees (MuJoCo's default 45). It looks along -z = -(x cross y)."""

    def __init__(self, pos: Sequence[float], xyaxes: Sequence[float], fovy: float = 45.0):
        pos = np.asarray(pos, np.float64).reshape(-1)
        ax = np.asarray(xyaxes, np.float64).reshape(-1)
        if pos.shape != (3,) or ax.shape != (6,):
            raise ValueError("Camera takes pos [3] and xyaxes [6]")
        if not (np.isfinite(pos).all() and np.isfinite(ax).all() and math.isfinite(fovy)):
            raise ValueError("Camera: non-finite pos, xyaxes or fovy")
        if not 0.0 < fovy < 180.0:
            raise ValueError(f"Camera: fovy must be inside (0, 180) degrees, got {fovy}")
        x, y = ax[:3], ax[3:]
        nx = np.linalg.norm(x)
        if not nx > 1e-9:
            raise ValueError("Camera: the x axis is zero")
        x = x / nx
        yo = y - (x @ y) * x
        ny = np.linalg.norm(yo)
        if not (ny > 1e-9 and ny > 1e-6 * np.linalg.norm(y)):
            raise ValueError("Camera: the y axis is zero or parallel to x")
        self.pos, self.x, self.y, self.fovy = pos, x, yo / ny, float(fovy)

    @property
    def z(self) -> np.ndarray:
        return np.cross(self.x, self.y)

    def desc(self) -> CameraDesc:
        return CameraDesc((C.c_double * 3)(*self.pos), (C.c_double * 3)(*self.x), (C.c_double * 3)(*self.y), self.fovy)

    def __repr__(self):
        return f"Camera(pos={self.pos.tolist()}, xyaxes={[*self.x.tolist(), *self.y.tolist()]}, fovy={self.fovy})"


_BASE_WIDTH_Y = 0.6105  # the piano base's half size along y (piano.py:132-141 pads it by 0.5 at distance 1)
# models/piano/piano.py:100-141, in its order (the index is dm_control's camera_id)
CAMERAS: Dict[str, Camera] = collections.OrderedDict([
    ("closeup", Camera((-0.313, 0.024, 0.455), (0.003, -1.000, -0.000, 0.607, 0.002, 0.795))),
    ("left", Camera((0.393, -0.791, 0.638), (0.808, 0.589, 0.000, -0.388, 0.533, 0.752))),
    ("right", Camera((0.472, 0.598, 0.580), (-0.637, 0.771, -0.000, -0.510, -0.421, 0.750))),
    ("back", Camera((-0.569, 0.008, 0.841), (-0.009, -1.000, 0.000, 0.783, -0.007, 0.622))),
    ("egocentric", Camera((0.417, -0.039, 0.717), (-0.002, 1.000, 0.000, -0.867, -0.002, 0.498))),
    # quat (1, 0, 0, 1): a quarter turn about z, so image x runs along world +y and it looks down
    ("topdown", Camera((0.0, 0.0, 1.0), (0.0, 1.0, 0.0, -1.0, 0.0, 0.0),
                       math.degrees(2.0 * math.atan2(0.5 * _BASE_WIDTH_Y, 1.0)))),
])


def camera_of(camera: Union[str, int, Camera]) -> Camera:
    """A name or an index of ``CAMERAS``, or a ``Camera`` as it is."""
    if isinstance(camera, Camera):
        return camera
    if isinstance(camera, str):
        if camera not in CAMERAS:
            raise ValueError(f"unknown camera {camera!r}; the piano's cameras are {list(CAMERAS)}")
        return CAMERAS[camera]
    if isinstance(camera, (int, np.integer)) and not isinstance(camera, bool):
        if not 0 <= camera < len(CAMERAS):
            raise ValueError(f"camera index {camera} outside 0 .. {len(CAMERAS) - 1} (the free camera -1 is not modelled)")
        return list(CAMERAS.values())[int(camera)]
    raise TypeError(f"camera must be a name, an index or a Camera, not {type(camera).__name__}")


def render(core, camera: Union[str, int, Camera] = "closeup", height: int = 240, width: int = 320, envs=None,
           depth: bool = False, segmentation: bool = False, change_color_on_activation: bool = False,
           colorize: Optional[bool] = None, count_list: bool = False):
    """``BatchedPianoEnv.render``: the envs ``envs`` (all N in order when None; any order, repeats
    allowed) through one camera, asynchronously on the current stream. Returns one tensor like
    dm_control's ``physics.render``: uint8 ``[n, H, W, 3]``, or with ``depth`` float32 ``[n, H, W]``
    (metres along the optical axis, +inf for a miss), or with ``segmentation`` int32 ``[n, H, W]``
    (collider id 0 .. 63, 64 + key, 152 base, 153 floor, -1 for a miss). ``colorize`` None means
    ``not task.disable_colorization``. An index outside [0, N) raises after the others' images
    were written (checking it synchronises; a call without ``envs`` does not)."""
    torch = core._torch
    if depth and segmentation:
        raise ValueError("render: depth and segmentation are exclusive (as in dm_control)")
    cam = camera_of(camera).desc()
    if colorize is None:
        colorize = not core.task.disable_colorization
    flags = (RENDER_ACTIVATION if change_color_on_activation else 0) | (RENDER_COLORIZE if colorize else 0) | \
        (RENDER_COUNT_LIST if count_list else 0)
    L = _lib.load()
    if not hasattr(L, "ps_render"):
        raise _lib.PianosimError("the loaded libpianosim has no ps_render (ps_version < 9)")
    sel = nbad = None
    n = core.num_envs
    if envs is not None:
        sel = torch.as_tensor(envs, device=core.device).to(torch.int32).reshape(-1).contiguous()
        n = int(sel.numel())
        nbad = torch.zeros(1, device=core.device, dtype=torch.int32)
    h, w = int(height), int(width)
    shape = (max(n, 0), max(h, 0), max(w, 0))
    rgb = dep = seg = None
    if depth:
        out = dep = torch.empty(shape, device=core.device, dtype=torch.float32)
    elif segmentation:
        out = seg = torch.empty(shape, device=core.device, dtype=torch.int32)
    else:
        out = rgb = torch.empty(shape + (3,), device=core.device, dtype=torch.uint8)
    ptr = lambda t: None if t is None else t.data_ptr()
    _lib.check(L.ps_render(core._h, C.byref(cam), w, h, ptr(sel), n, flags, ptr(rgb), ptr(dep), ptr(seg), ptr(nbad),
                           core.stream))
    core._render_keep = (sel, nbad)  # alive until the kernels ran
    if nbad is not None and int(nbad.item()):
        raise _lib.PianosimError(f"render: {int(nbad.item())} env indices outside [0, {core.num_envs}); their images "
                                 "were left unwritten")
    return out


def list_stats(core, reset: bool = True):
    """(summed tile-list lengths, tiles) of the renders with ``count_list`` since the last reset."""
    out = (C.c_uint64 * 2)()
    _lib.check(_lib.load().ps_render_list_stats(core._h, out, int(reset)))
    return int(out[0]), int(out[1])


class Physics:
    """``Environment.physics``: the part of dm_control's ``Physics`` that looks at the env."""

    def __init__(self, core):
        self._core = core

    def render(self, height: int = 240, width: int = 320, camera_id: Union[str, int, Camera] = "closeup",
               depth: bool = False, segmentation: bool = False, change_color_on_activation: bool = False,
               colorize: Optional[bool] = None) -> np.ndarray:
        """``physics.render``: env 0 as a numpy array ``[H, W, 3]`` uint8 (``[H, W]`` float32 depth
        or int32 segmentation). ``camera_id``: a name or index of ``CAMERAS`` or a ``Camera``."""
        out = render(self._core, camera_id, height, width, None if self._core.num_envs == 1 else [0], depth,
                     segmentation, change_color_on_activation, colorize)
        return out[0].cpu().numpy()


class PixelWrapper:
    """``robopianist.wrappers.PixelWrapper``: adds the rendered image to the observation under
    ``observation_key``. Over an ``Environment`` (anything with ``physics.render`` and dm_env
    ``TimeStep`` s) the key holds ``[H, W, 3]``; over a ``VectorizedPianoEnv`` every env's image,
    ``[N, H, W, 3]``, as a torch tensor (numpy with ``return_numpy``). ``render_kwargs`` are
    ``physics.render``'s (``camera_id``, ``height``, ``width``, ...)."""

    def __init__(self, environment, render_kwargs: Optional[Dict[str, Any]] = None, observation_key: str = "pixels"):
        self._environment = environment
        self._render_kwargs = dict(render_kwargs or {})
        self._observation_key = observation_key
        self._batched = not hasattr(environment, "physics")
        if self._batched and not hasattr(getattr(environment, "core", None), "render"):
            raise TypeError("PixelWrapper needs an environment with physics.render, or a VectorizedPianoEnv")
        spec = environment.observation_spec
        wrapped = spec() if callable(spec) else spec
        if observation_key in wrapped:
            raise ValueError(f"the observation already has a key {observation_key!r}")
        from .envs import Array
        pixels = self._pixels()
        self._observation_spec = collections.OrderedDict(wrapped)
        self._observation_spec[observation_key] = Array(tuple(pixels.shape), _np_dtype(pixels), observation_key)

    def _pixels(self):
        if not self._batched:
            return self._environment.physics.render(**self._render_kwargs)
        kw = dict(self._render_kwargs)
        if "camera_id" in kw:
            kw["camera"] = kw.pop("camera_id")
        out = self._environment.core.render(**kw)
        return out.cpu().numpy() if getattr(self._environment, "return_numpy", False) else out

    def observation_spec(self):
        return self._observation_spec

    def _add(self, observation):
        return collections.OrderedDict(observation, **{self._observation_key: self._pixels()})

    def reset(self):
        out = self._environment.reset()
        return self._add(out) if self._batched else out._replace(observation=self._add(out.observation))

    def step(self, action):
        out = self._environment.step(action)
        if self._batched:
            return (self._add(out[0]),) + tuple(out[1:])
        return out._replace(observation=self._add(out.observation))

    def __getattr__(self, name):
        return getattr(self._environment, name)


def _np_dtype(a):
    return a.dtype if isinstance(a, np.ndarray) else np.dtype(str(a.dtype).replace("torch.", ""))


def _chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def write_png(path, image) -> None:
    """``image`` uint8 ``[H, W, 3]`` (RGB) or ``[H, W]`` (grey), numpy or torch, as an 8-bit PNG."""
    if hasattr(image, "detach"):
        image = image.detach().cpu().numpy()
    a = np.asarray(image)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3) or a.size == 0:
        raise ValueError(f"write_png takes a uint8 [H, W, 3] or [H, W] image, got {a.dtype} {a.shape}")
    h, w = a.shape[:2]
    rows = np.ascontiguousarray(a).reshape(h, -1)
    raw = np.concatenate([np.zeros((h, 1), np.uint8), rows], axis=1).tobytes()  # filter 0 on every row
    ihdr = struct.pack(">IIBBBBB", w, h, 8, 2 if a.ndim == 3 else 0, 0, 0, 0)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(raw, 6)) +
                _chunk(b"IEND", b""))
