"""Device-side preprocessing of the inference surface (``zoo.encode``): job tables on the host, one kernel on the device.

The reference's ``encode`` prepares every image on the host (zoo/encode.py:34-72,129-157): HU conversion, window, three PIL
bilinear resizes, normalise.  ``csrc/encode_prep.hip`` (``dinox_encode_preprocess``) restates that on the device.  Its unit of
work is a *plane job*: one source plane, filtered once, written to up to three ``(image, channel)`` destinations.  This module
builds the job tables -- ``plane_jobs`` for a list of images of mixed shapes, ``volume_jobs`` for the 2.5D stacks of a
``(Z, H, W)`` volume -- and launches the kernel (``device_preprocess``).  Everything but the launch runs without a GPU.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

JOB_FIELDS = 9                  # offset, H, W, row stride, pixel stride, n destinations, 3 destinations (image * 3 + channel, -1: unused)
FORMATS = ("hu_float", "hu16_png", "windowed_float")
CONTEXTS = ("neighbours", "replicate")
_KERNEL_DTYPES = ("uint16", "int16", "float32")       # what the kernel reads; anything else is converted to float32 while packing


class PreprocessUnsupported(RuntimeError):
    """The kernel declined (DINOX_EUNSUPPORTED): nothing was launched.  ``preprocess="auto"`` falls back to the host on this."""


def source_dtype(arr: np.ndarray) -> str:
    """Name of the packed buffer an array goes to."""
    return arr.dtype.name if arr.dtype.name in _KERNEL_DTYPES else "float32"


@dataclass
class SourceLayout:
    """Where ``plane_jobs`` puts every image: one flat buffer per source dtype, images C-contiguous in their own shape, in list order.
    ``placements[i] = (dtype name, element offset, shape)`` of image i; ``sizes[dtype]`` = elements of that buffer;
    ``job_dtype[j]`` = the buffer job j reads (offsets in the job table count elements of THAT buffer)."""
    placements: List[Tuple[str, int, Tuple[int, ...]]] = field(default_factory=list)
    sizes: Dict[str, int] = field(default_factory=dict)
    job_dtype: List[str] = field(default_factory=list)

    def jobs_of(self, jobs: np.ndarray, dtype: str) -> np.ndarray:
        return jobs[[i for i, d in enumerate(self.job_dtype) if d == dtype]]


def _planes(shape: Tuple[int, ...]) -> List[Tuple[int, int, int, int, int]]:
    """(offset, H, W, row stride, pixel stride) of the three channel planes of a C-contiguous image, in the order of
    ``zoo.encode._channels``; one entry for an (H, W) image."""
    if len(shape) == 2:
        H, W = shape
        return [(0, H, W, W, 1)]
    if len(shape) == 3 and shape[2] == 3:
        H, W = shape[0], shape[1]
        return [(c, H, W, 3 * W, 3) for c in range(3)]
    if len(shape) == 3 and shape[0] == 3:
        H, W = shape[1], shape[2]
        return [(c * H * W, H, W, W, 1) for c in range(3)]
    raise ValueError(f"Unsupported image shape: {tuple(shape)}. Expected (H, W), (H, W, 3), or (3, H, W).")


def plane_jobs(images: Sequence[np.ndarray]) -> Tuple[np.ndarray, SourceLayout, int]:
    """Job table of a list of images of shapes (H, W), (H, W, 3) and (3, H, W): ``(jobs int64 [n_jobs, 9], layout, max_side)``.
    An (H, W) image is ONE job with three destinations (the reference replicates the plane); a three-channel image is three jobs.
    Jobs come in image order, so ``layout.job_dtype`` groups them into one launch per source dtype."""
    layout = SourceLayout()
    rows, max_side = [], 1
    for i, im in enumerate(images):
        shape = tuple(int(v) for v in np.shape(im))
        planes = _planes(shape)
        if min(shape) < 1:
            raise ValueError(f"Unsupported image shape: {shape}. Expected (H, W), (H, W, 3), or (3, H, W).")
        dt = source_dtype(np.asarray(im))
        base = layout.sizes.get(dt, 0)
        layout.placements.append((dt, base, shape))
        layout.sizes[dt] = base + int(np.prod(shape))
        for c, (off, H, W, rs, ps) in enumerate(planes):
            dests = [3 * i, 3 * i + 1, 3 * i + 2] if len(planes) == 1 else [3 * i + c, -1, -1]
            rows.append((base + off, H, W, rs, ps, 3 if len(planes) == 1 else 1, *dests))
            layout.job_dtype.append(dt)
            max_side = max(max_side, H, W)
    return np.asarray(rows, dtype=np.int64).reshape(-1, JOB_FIELDS), layout, max_side


def stack_planes(Z: int, z: int, context: str) -> Tuple[int, int, int]:
    """The planes of the 2.5D stack of slice z (reference scripts/phase5_big_run.py:535-545: z-1, z, z+1 clamped to the series)."""
    if context == "replicate":
        return (z, z, z)
    return (max(z - 1, 0), z, min(z + 1, Z - 1))


def volume_jobs(Z: int, H: int, W: int, z_indices: Sequence[int], context: str = "neighbours") -> np.ndarray:
    """Job table for slices ``z_indices`` of a C-contiguous (Z, H, W) volume; image k of the batch is slice ``z_indices[k]``.
    Every plane any requested stack shows is ONE job carrying all its (image, channel) destinations -- one resize per plane
    instead of three -- split into further jobs where more than three want it (repeated or clamped slices)."""
    if context not in CONTEXTS:
        raise ValueError(f"Unknown context: '{context}'. Supported: 'neighbours', 'replicate'")
    wanted: Dict[int, List[int]] = {}
    for k, z in enumerate(z_indices):
        z = int(z)
        if not 0 <= z < Z:
            raise ValueError(f"slice index {z} outside a volume of {Z} slices")
        for c, plane in enumerate(stack_planes(Z, z, context)):
            wanted.setdefault(plane, []).append(3 * k + c)
    rows = []
    for plane in sorted(wanted):
        dests = wanted[plane]
        for at in range(0, len(dests), 3):
            part = dests[at:at + 3]
            rows.append((plane * H * W, H, W, W, 1, len(part), *(part + [-1] * (3 - len(part)))))
    return np.asarray(rows, dtype=np.int64).reshape(-1, JOB_FIELDS)


def volume_tile_jobs(Z: int, H: int, W: int, items: Sequence[Tuple[int, int, int]], t: int, context: str = "neighbours") -> np.ndarray:
    """``volume_jobs`` for t x t tiles: image k of the batch is the crop at rows [y0, y0 + t), columns [x0, x0 + t) of the 2.5D stack of
    slice z, ``items[k] = (z, y0, x0)``.  A crop is a job like any other -- offset plane H W + y0 W + x0, size t x t, row stride W -- and
    every plane crop any requested stack shows is ONE job with all its destinations (further jobs where more than three want it)."""
    if context not in CONTEXTS:
        raise ValueError(f"Unknown context: '{context}'. Supported: 'neighbours', 'replicate'")
    if int(t) != t or not 1 <= t <= min(H, W):
        raise ValueError(f"tile side {t!r} outside [1, min(H, W) = {min(H, W)}]")
    t = int(t)
    wanted: Dict[Tuple[int, int, int], List[int]] = {}
    for k, (z, y0, x0) in enumerate(items):
        z, y0, x0 = int(z), int(y0), int(x0)
        if not 0 <= z < Z:
            raise ValueError(f"slice index {z} outside a volume of {Z} slices")
        if not (0 <= y0 <= H - t and 0 <= x0 <= W - t):
            raise ValueError(f"tile at ({y0}, {x0}) of side {t} reaches past a {H} x {W} plane")
        for c, plane in enumerate(stack_planes(Z, z, context)):
            wanted.setdefault((plane, y0, x0), []).append(3 * k + c)
    rows = []
    for plane, y0, x0 in sorted(wanted):
        dests = wanted[(plane, y0, x0)]
        for at in range(0, len(dests), 3):
            part = dests[at:at + 3]
            rows.append((plane * H * W + y0 * W + x0, t, t, W, 1, len(part), *(part + [-1] * (3 - len(part)))))
    return np.asarray(rows, dtype=np.int64).reshape(-1, JOB_FIELDS)


def check_jobs(jobs: np.ndarray, src_numel: int, n_images: int) -> int:
    """Host-side bounds check of a job table against its source buffer (the kernel trusts the table); returns max_side."""
    jobs = np.asarray(jobs)
    if jobs.ndim != 2 or jobs.shape[1] != JOB_FIELDS or jobs.shape[0] < 1 or jobs.dtype != np.int64:
        raise ValueError(f"job table must be int64 [n_jobs >= 1, {JOB_FIELDS}], got {jobs.dtype} {jobs.shape}")
    off, H, W, rs, ps, nd = (jobs[:, i] for i in range(6))
    if (off < 0).any() or (H < 1).any() or (W < 1).any() or (rs < 1).any() or (ps < 1).any():
        raise ValueError("job table: negative offset or non-positive size / stride")
    if (off + (H - 1) * rs + (W - 1) * ps >= src_numel).any():
        raise ValueError(f"job table reaches past the source buffer ({src_numel} elements)")
    if (nd < 1).any() or (nd > 3).any():
        raise ValueError("job table: 1 to 3 destinations per job")
    d = jobs[:, 6:9]
    used = np.arange(3)[None, :] < nd[:, None]
    if (d[used] < 0).any() or (d[used] >= 3 * n_images).any():
        raise ValueError(f"job table: destination outside the {n_images} images of the batch")
    return int(max(H.max(), W.max()))


def _dtype_code(t: torch.Tensor, src_dtype: Optional[str]) -> int:
    from . import _lib
    name = src_dtype or str(t.dtype).replace("torch.", "")
    if name == "float32" and t.dtype == torch.float32:
        return _lib.F32
    if name in ("uint16", "int16") and t.dtype in (torch.int16, torch.uint16):       # 16-bit storage carries either bit pattern
        return _lib.U16 if name == "uint16" else _lib.I16
    raise TypeError(f"source tensor {t.dtype} read as {name}: the kernel takes uint16, int16 and float32")


def device_preprocess(src_tensor: torch.Tensor, jobs, n_images: int, S: int, fmt: str, level: float, width: float,
                      out: Optional[torch.Tensor] = None, *, src_dtype: Optional[str] = None,
                      max_side: Optional[int] = None) -> torch.Tensor:
    """Launch ``dinox_encode_preprocess`` on the current stream: (n_images, 3, S, S) fp32 on the device of ``src_tensor``.
    ``jobs``: a host table (ndarray / CPU tensor: checked against the buffer, then copied through page-locked memory) or a table
    already on the device (trusted; pass ``max_side``).  ``src_dtype`` ("uint16" / "int16") says how a 16-bit buffer is read.
    Destinations no job names keep what ``out`` held.  Raises ``PreprocessUnsupported`` when the kernel declines."""
    from . import _lib, ops
    if fmt not in FORMATS:
        raise ValueError(f"Unknown input_format: '{fmt}'. Supported: 'hu_float', 'hu16_png', 'windowed_float'")
    ops._need_cuda(src_tensor)
    assert src_tensor.is_contiguous()
    code = _dtype_code(src_tensor, src_dtype)
    dev = src_tensor.device
    if isinstance(jobs, torch.Tensor) and jobs.is_cuda:
        assert max_side is not None and jobs.dtype == torch.int64 and jobs.is_contiguous() and jobs.dim() == 2 and jobs.shape[1] == JOB_FIELDS
        jobs_dev = jobs
    else:
        table = np.ascontiguousarray(jobs.numpy() if isinstance(jobs, torch.Tensor) else jobs)
        max_side = check_jobs(table, src_tensor.numel(), n_images)
        jobs_dev = torch.from_numpy(table).pin_memory().to(dev, non_blocking=True)
    if out is None:
        out = torch.empty((n_images, 3, S, S), dtype=torch.float32, device=dev)
    else:
        assert out.shape == (n_images, 3, S, S) and out.dtype == torch.float32 and out.is_contiguous() and out.device == dev
    lo, hi = level - width / 2, level + width / 2           # in double, as the reference computes them
    rc = launch(ops._p(src_tensor), code, ops._p(jobs_dev), int(jobs_dev.shape[0]), ops._p(out), n_images, S, int(max_side), lo, hi,
                FORMATS.index(fmt), ops._stream())
    if rc == _lib.EUNSUPPORTED:
        raise PreprocessUnsupported(f"dinox_encode_preprocess declined (code {rc}): {_lib.last_error()}")
    _lib.check(rc, "dinox_encode_preprocess")
    return out


def launch(*args) -> int:
    """The library call itself (a seam of its own: everything above it is host logic)."""
    from ._lib import lib
    return lib.dinox_encode_preprocess(*args)


def lds_bytes(S: int, max_side: int) -> int:
    from ._lib import lib
    return int(lib.dinox_encode_preprocess_lds_bytes(S, max_side))


# ---------------------------------------------------------------- packing a list of host arrays
_staging: Dict[str, Tuple[torch.Tensor, Optional[torch.cuda.Event]]] = {}     # one page-locked buffer per dtype, grown on demand


def _staging_buffer(dtype: str, numel: int) -> torch.Tensor:
    tdt = torch.float32 if dtype == "float32" else torch.int16
    buf, ev = _staging.get(dtype, (None, None))
    if ev is not None:
        ev.synchronize()                                    # the copy that last read this buffer
    if buf is None or buf.numel() < numel:
        buf = torch.empty(int(numel * 1.25) + 1024, dtype=tdt, pin_memory=True)
    _staging[dtype] = (buf, None)
    return buf


def pack_and_preprocess(images: Sequence[np.ndarray], S: int, fmt: str, level: float, width: float, device,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The device path of ``encode`` / ``encode_batch``: the raw arrays go, as they are (strided input is gathered, other dtypes
    become float32), into one page-locked buffer per source dtype; one copy and one launch per dtype fill (B, 3, S, S)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"dinox: preprocess='device' needs a CUDA/HIP device, not '{device}' -- the kernel library is the only "
                           "compute path. Move the model to 'cuda' or use preprocess='host'.")
    jobs, layout, _ = plane_jobs(images)
    n = len(images)
    if out is None:
        out = torch.empty((n, 3, S, S), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        for dt, numel in layout.sizes.items():
            buf = _staging_buffer(dt, numel)
            host = buf.numpy()[:numel]
            if dt == "uint16":
                host = host.view(np.uint16)
            for im, (d, off, shape) in zip(images, layout.placements):
                if d == dt:
                    np.copyto(host[off:off + int(np.prod(shape))].reshape(shape), np.asarray(im), casting="unsafe")
            src = buf[:numel].to(device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            _staging[dt] = (buf, ev)
            device_preprocess(src, layout.jobs_of(jobs, dt), n, S, fmt, level, width, out=out, src_dtype=dt)
    return out
