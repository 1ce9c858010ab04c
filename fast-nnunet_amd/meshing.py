"""Surface models of a label map: one closed triangle surface per label or region, made on the GPU by ``fnn_mesh_count`` /
``fnn_mesh_emit`` (csrc/mesh.hip), thinned there by ``fnn_mesh_decimate`` (csrc/mesh_decimate.hip), and a legacy-VTK
PolyData writer for them.

This is what the reference's front end calls ``VTKModelGenerator(color_file_path=...).generate_vtk_model(mask_path=...,
output_path=..., smoothing_factor=0.5, decimation_factor=0.2)`` for.  The generator's own source is not part of the
reference, so the surface is this project's definition (include/fnn.h states it): the voxel faces between a region and
everything else, Taubin-smoothed on the lattice graph, in world coordinates.  Differences a caller of the reference meets:

* ``smoothing_factor`` s in [0, 1] means ``round(PAIRS_AT_FACTOR_ONE * s)`` Taubin pairs (f = 0.5, then f = -0.53);
* ``decimation_factor`` d in [0, 1) asks for ceil((1 - d) * triangles) triangles by rounds of quadric-error edge collapse
  on the GPU (include/fnn.h states the rule); a surface whose non-manifold edges leave no candidate stops early and says so
  (``exhausted``).  ``label_surfaces`` and ``decimate_surfaces`` take it; ``VTKModelGenerator`` honours it when it is made
  with ``decimation=True`` and otherwise still raises NotImplementedError for a factor other than 0 (the reference passes
  0.2), so that nobody gets a decimated model without asking;
* no foreign reader has opened the files: ``read_vtk_polydata`` reads exactly what ``write_vtk_polydata`` makes.

Colours: a region takes the colour of its smallest label id from the colour table (``read_color_table``: the reference's
``id name r g b a`` lines); an id the table lacks, or any id without a table, gets ``fallback_color(id)``: hue
frac(id * 0.6180339887498949) at full saturation and value, every channel round(255 c), alpha 255, name ``label_<id>``.

There is no CPU path: the surfaces are made by the HIP library on an AMD GPU."""
from __future__ import annotations

import colorsys
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import capi
from .evaluation import _device, _members, check_label_map

PAIRS_AT_FACTOR_ONE = 50                    # Taubin pairs at smoothing_factor 1.0 (this project's mapping)
MAX_REGIONS = 1024
_GOLDEN = 0.6180339887498949
VTK_TITLE = 'fast-nnunet_amd surface model'


@dataclass
class SurfaceModel:
    """points float32 [n, 3] (world x, y, z); triangles int32 [m, 3] into points; triangle_region uint16 [m]: the index
    into ``regions`` (tuples of label ids); region k owns points[point_offsets[k]:point_offsets[k + 1]] and
    triangles[triangle_offsets[k]:triangle_offsets[k + 1]].  rounds, exhausted: what a decimation reported (exhausted: it
    stopped above its target because no edge could be collapsed any more, or at its limit of rounds)."""
    points: np.ndarray
    triangles: np.ndarray
    triangle_region: np.ndarray
    regions: List[Tuple[int, ...]]
    point_offsets: np.ndarray
    triangle_offsets: np.ndarray
    rounds: int = 0
    exhausted: int = 0


def smoothing_pairs(smoothing_factor: float) -> int:
    s = float(smoothing_factor)
    if not 0.0 <= s <= 1.0:                                         # (a NaN fails both comparisons)
        raise ValueError(f'smoothing_factor must lie in [0, 1], got {smoothing_factor}')
    return int(round(PAIRS_AT_FACTOR_ONE * s))


def check_decimation(decimation_factor: float) -> float:
    d = float(decimation_factor)
    if not 0.0 <= d < 1.0:                                          # (a NaN fails both comparisons)
        raise ValueError(f'decimation_factor must lie in [0, 1), got {decimation_factor}')
    return d


def fallback_color(label_id: int) -> Tuple[str, int, int, int, int]:
    """(name, r, g, b, a) of an id without a table entry - the rule in this module's docstring."""
    r, g, b = colorsys.hsv_to_rgb((int(label_id) * _GOLDEN) % 1.0, 1.0, 1.0)
    return (f'label_{int(label_id)}', int(round(255 * r)), int(round(255 * g)), int(round(255 * b)), 255)


def read_color_table(path: str) -> Dict[int, Tuple[str, int, int, int, int]]:
    """The reference's colour table (``id name r g b a`` per line, ``#`` starts a comment) -> {id: (name, r, g, b, a)}."""
    table = {}
    with open(path, 'r', encoding='utf-8') as f:
        for no, line in enumerate(f, 1):
            text = line.split('#', 1)[0].strip()
            if not text:
                continue
            parts = text.split()
            try:
                if len(parts) != 6:
                    raise ValueError('expected 6 fields')
                lid, rgba = int(parts[0]), tuple(int(p) for p in parts[2:])
                if lid < 0 or any(c < 0 or c > 255 for c in rgba):
                    raise ValueError('id or colour out of range')
            except ValueError as e:
                raise ValueError(f'{path}:{no}: not an "id name r g b a" line ({e}): {line.rstrip()!r}') from None
            table[lid] = (parts[1],) + rgba
    return table


def region_colors(regions: Sequence[Sequence[int]], table: Optional[dict] = None) -> np.ndarray:
    """uint8 [n_regions, 4]: the colour of every region's smallest label id."""
    out = np.zeros((len(regions), 4), np.uint8)
    for k, r in enumerate(regions):
        lid = min(r)
        out[k] = (table[lid] if table and lid in table else fallback_color(lid))[1:]
    return out


def _check_affine(affine, spacing, coordinate_system: str) -> np.ndarray:
    if affine is not None and spacing is not None:
        raise ValueError('give affine or spacing, not both')
    if coordinate_system not in ('RAS', 'LPS'):
        raise ValueError(f"coordinate_system must be 'RAS' or 'LPS', got {coordinate_system!r}")
    if spacing is not None:
        sp = np.asarray(spacing, np.float64).reshape(-1)
        if sp.shape != (3,) or not np.all(np.isfinite(sp)) or not np.all(sp > 0):
            raise ValueError(f'spacing must be three finite positive numbers (z, y, x), got {spacing}')
        a = np.diag([sp[2], sp[1], sp[0], 1.0])
    elif affine is None:
        a = np.eye(4)
    else:
        a = np.array(affine, np.float64)
        if a.shape != (4, 4):
            raise ValueError(f'the affine must be 4x4, got shape {a.shape}')
        if not np.all(np.isfinite(a)):
            raise ValueError('the affine must be finite')
        if not abs(np.linalg.det(a[:3, :3])) > 0.0:
            raise ValueError('the affine must be invertible')
    if coordinate_system == 'LPS':
        a[:2] = -a[:2]
    return a


def _check_regions(labels_or_regions) -> List[Tuple[int, ...]]:
    regions = [tuple(_members(r)) for r in labels_or_regions]
    for r in regions:
        if not r:
            raise ValueError('a region without label ids')
        for v in r:
            if v < 0 or v > 65535:
                raise ValueError(f'label {v} is outside 0..65535')
    if len(regions) > MAX_REGIONS:
        raise ValueError(f'at most {MAX_REGIONS} labels or regions make one model, got {len(regions)}')
    return regions


def _member_table(regions: Sequence[Sequence[int]]) -> np.ndarray:
    member = np.zeros((len(regions), max(v for r in regions for v in r) + 1), np.uint8)
    for k, r in enumerate(regions):
        member[k, list(r)] = 1
    return member


def _check_map(seg) -> int:
    """The refusals of a label map before any GPU call; -> its largest value (int16 device tensors carry uint16 bits)."""
    shape = tuple(seg.shape) if isinstance(seg, torch.Tensor) else np.shape(seg)
    if isinstance(seg, torch.Tensor):
        if seg.dtype == torch.bool or seg.dtype.is_floating_point or seg.dtype.is_complex:
            raise ValueError(f'label maps must have an integer dtype, got {seg.dtype}')
    elif np.asarray(seg).dtype.kind not in 'iu':
        raise ValueError(f'label maps must have an integer dtype, got {np.asarray(seg).dtype}')
    if len(shape) != 3:
        raise ValueError(f'surfaces are made from 3-D label maps (z, y, x), got shape {shape}')
    if isinstance(seg, torch.Tensor) and seg.dtype in (torch.int16, torch.uint16):
        return int((seg.view(torch.int16).to(torch.int32) & 0xFFFF).max()) if seg.numel() else 0
    return check_label_map(seg)[1]


def _to_device(seg, top: int, dev: torch.device) -> torch.Tensor:
    """A contiguous device tensor (z, y, x) of uint8, or of int16 that carries uint16 bits; a device map of those types is
    used where it lies."""
    if isinstance(seg, torch.Tensor):
        t = seg if seg.device.type == 'cuda' else seg.to(dev)
        if t.dtype == torch.uint16:
            t = t.view(torch.int16)
    else:
        arr = np.asarray(seg)
        arr = arr.astype(np.uint8) if top < 256 else arr.astype(np.uint16).view(np.int16)
        t = torch.from_numpy(np.ascontiguousarray(arr)).to(dev)
    if t.dtype not in (torch.uint8, torch.int16):
        t = t.to(torch.uint8) if top < 256 else t.to(torch.int32).to(torch.int16)
    return t.contiguous()


class _DeviceMesh:
    """The buffers one fnn_mesh_emit call filled."""

    def __init__(self, seg: torch.Tensor, regions, affine: np.ndarray, pairs: int, layout: int):
        dev = seg.device
        u16 = seg.dtype == torch.int16
        self.regions, self.layout = regions, layout
        stream = torch.cuda.current_stream(dev).cuda_stream
        if regions:
            member = _member_table(regions)
            self.counts, self.boxes = capi.mesh_count(seg.data_ptr(), u16, seg.shape, member, stream)
        else:
            self.counts, self.boxes = np.zeros((0, 2), np.int64), np.zeros((0, 6), np.int64)
        self.point_offsets = np.concatenate([[0], np.cumsum(self.counts[:, 0])]).astype(np.int64)
        self.triangle_offsets = np.concatenate([[0], np.cumsum(2 * self.counts[:, 1])]).astype(np.int64)
        n, t = int(self.point_offsets[-1]), int(self.triangle_offsets[-1])
        self.n, self.t = n, t
        self.triangle_counts = 2 * self.counts[:, 1]
        self.rounds = self.exhausted = 0
        self.points = torch.empty(max(n, 1) * 12, dtype=torch.uint8, device=dev)
        self.cells = torch.empty(max(t, 1) * (16 if layout else 12), dtype=torch.uint8, device=dev)
        self.cell_region = torch.empty(max(t, 1) * 2, dtype=torch.uint8, device=dev)
        if t:
            capi.mesh_emit(seg.data_ptr(), u16, seg.shape, member, affine, pairs, layout, self.points.data_ptr(), n,
                           self.cells.data_ptr(), t, self.cell_region.data_ptr(), stream)

    def decimated(self, decimation_factor: float, layout: int) -> '_DeviceMesh':
        """fnn_mesh_decimate of this layout-0 mesh into buffers of their own, in ``layout``."""
        assert self.layout == 0
        out = object.__new__(_DeviceMesh)
        out.regions, out.layout, out.boxes = self.regions, layout, self.boxes
        out.points, out.cell_region = torch.empty_like(self.points), torch.empty_like(self.cell_region)
        out.cells = torch.empty(max(self.t, 1) * (16 if layout else 12), dtype=torch.uint8, device=self.points.device)
        counts, out.n, out.t, out.rounds, out.exhausted = capi.mesh_decimate(
            self.points.data_ptr(), self.n, self.cells.data_ptr(), self.cell_region.data_ptr(), self.t, self.point_offsets, decimation_factor,
            layout, out.points.data_ptr(), self.n, out.cells.data_ptr(), self.t, out.cell_region.data_ptr(),
            torch.cuda.current_stream(self.points.device).cuda_stream)
        out.counts, out.triangle_counts = counts, counts[:, 1].copy()
        out.point_offsets = np.concatenate([[0], np.cumsum(counts[:, 0])]).astype(np.int64)
        out.triangle_offsets = np.concatenate([[0], np.cumsum(counts[:, 1])]).astype(np.int64)
        return out

    def payload(self) -> Tuple[bytes, bytes, bytes]:
        return (self.points[:self.n * 12].cpu().numpy().tobytes(), self.cells[:self.t * (16 if self.layout else 12)].cpu().numpy().tobytes(),
                self.cell_region[:self.t * 2].cpu().numpy().tobytes())


def _present_labels(seg: torch.Tensor, top: int) -> List[Tuple[int, ...]]:
    """Every foreground value of the map: the labels 1..top that fnn_mesh_count finds a face of."""
    stream = torch.cuda.current_stream(seg.device).cuda_stream
    present = []
    for lo in range(1, top + 1, MAX_REGIONS):
        ids = list(range(lo, min(lo + MAX_REGIONS, top + 1)))
        counts, _ = capi.mesh_count(seg.data_ptr(), seg.dtype == torch.int16, seg.shape, _member_table([(v,) for v in ids]), stream)
        present += [(v,) for v, c in zip(ids, counts[:, 1]) if c]
    if len(present) > MAX_REGIONS:
        raise ValueError(f'at most {MAX_REGIONS} labels or regions make one model, the map holds {len(present)} labels')
    return present


def _device_mesh(seg, labels_or_regions, a: np.ndarray, pairs: int, layout: int, device=None, decimation: float = 0.0) -> _DeviceMesh:
    regions = None if labels_or_regions is None else _check_regions(labels_or_regions)
    top = _check_map(seg)
    dev = seg.device if isinstance(seg, torch.Tensor) and seg.device.type == 'cuda' else (torch.device(device) if device is not None else _device())
    with torch.cuda.device(dev):
        t = _to_device(seg, top, dev)
        if regions is None:
            regions = _present_labels(t, top) if t.numel() else []
        if decimation == 0.0:
            return _DeviceMesh(t, regions, a, pairs, layout)
        return _DeviceMesh(t, regions, a, pairs, 0).decimated(decimation, layout)   # emitted in layout 0, decimated into `layout`


def label_surfaces(seg, labels_or_regions=None, affine=None, spacing=None, smoothing_factor: float = 0.0,
                   coordinate_system: str = 'RAS', decimation_factor: float = 0.0) -> SurfaceModel:
    """The surfaces of a label map (z, y, x; numpy, or a torch tensor that is used where it lies when it is on the GPU) as a
    ``SurfaceModel``.  ``labels_or_regions``: label ids or tuples of ids, None for every foreground value present.  Give a 4x4
    ``affine`` from index (x, y, z) to world, or a ``spacing`` (z, y, x) for diag(sx, sy, sz), or neither for the identity.
    ``coordinate_system='LPS'`` negates the first two world axes.  An int16 device tensor carries uint16 bits.
    ``decimation_factor`` d in [0, 1): the model is decimated on the device to ceil((1 - d) * triangles) triangles before it
    is downloaded; 0 makes the GPU calls of a plain surface."""
    pairs = smoothing_pairs(smoothing_factor)
    d = check_decimation(decimation_factor)
    a = _check_affine(affine, spacing, coordinate_system)
    return _model_of(_device_mesh(seg, labels_or_regions, a, pairs, 0, decimation=d))


def _model_of(m: _DeviceMesh) -> SurfaceModel:
    pts, cells, reg = m.payload()
    return SurfaceModel(np.frombuffer(pts, np.float32).reshape(-1, 3).copy(), np.frombuffer(cells, np.int32).reshape(-1, 3).copy(),
                        np.frombuffer(reg, np.uint16).copy(), list(m.regions), m.point_offsets, m.triangle_offsets, m.rounds, m.exhausted)


def decimate_surfaces(model: SurfaceModel, decimation_factor: float, device=None) -> SurfaceModel:
    """``model`` with ceil((1 - decimation_factor) * triangles) triangles (fnn_mesh_decimate): what
    ``label_surfaces(..., decimation_factor=...)`` gives for the map the model was made from."""
    d = check_decimation(decimation_factor)
    points = np.ascontiguousarray(model.points, np.float32).reshape(-1, 3)
    triangles = np.ascontiguousarray(model.triangles, np.int32).reshape(-1, 3)
    region = np.ascontiguousarray(model.triangle_region, np.uint16).reshape(-1)
    offsets = np.asarray(model.point_offsets, np.int64).reshape(-1)
    if len(region) != len(triangles) or len(offsets) != len(model.regions) + 1 or offsets[0] != 0 or offsets[-1] != len(points):
        raise ValueError('the model\'s triangle_region or point_offsets do not fit its points, triangles and regions')
    if len(triangles) and (triangles.min() < 0 or triangles.max() >= len(points) or (len(region) and region.max() >= len(model.regions))):
        raise ValueError('a triangle of the model names a point or a region that is not there')
    dev = torch.device(device) if device is not None else _device()
    with torch.cuda.device(dev):
        m = object.__new__(_DeviceMesh)
        m.regions, m.layout, m.boxes, m.n, m.t = list(model.regions), 0, None, len(points), len(triangles)
        up = lambda arr: torch.from_numpy(np.frombuffer(arr.tobytes() or b'\0', np.uint8).copy()).to(dev)
        m.points, m.cells, m.cell_region, m.point_offsets = up(points), up(triangles), up(region), offsets
        return _model_of(m.decimated(d, 0))


def _vtk_file(path: str, n: int, t: int, points: bytes, cells: bytes, labels: np.ndarray, colors: np.ndarray) -> None:
    """The legacy-VTK binary PolyData file from big-endian payloads; it appears under its name only when it is complete."""
    tmp = f'{path}.part{os.getpid()}'
    try:
        with open(tmp, 'wb') as f:
            f.write(f'# vtk DataFile Version 3.0\n{VTK_TITLE}\nBINARY\nDATASET POLYDATA\n'.encode('ascii'))
            f.write(f'POINTS {n} float\n'.encode('ascii'))
            f.write(points)
            f.write(f'\nPOLYGONS {t} {4 * t}\n'.encode('ascii'))
            f.write(cells)
            f.write(f'\nCELL_DATA {t}\nSCALARS label unsigned_short 1\nLOOKUP_TABLE default\n'.encode('ascii'))
            f.write(np.ascontiguousarray(labels, '>u2').tobytes())
            f.write(b'\nCOLOR_SCALARS colors 4\n')
            f.write(np.ascontiguousarray(colors, np.uint8).tobytes())
            f.write(b'\n')
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def _cell_data(regions, triangle_counts, colors) -> Tuple[np.ndarray, np.ndarray]:
    """Per triangle the smallest label id of its region and its colour; ``colors``: None, a colour table, or uint8 [R, 4]."""
    if isinstance(colors, np.ndarray):
        rc = np.asarray(colors, np.uint8).reshape(len(regions), 4)
    else:
        rc = region_colors(regions, colors)
    ids = np.array([min(r) for r in regions], np.uint16)
    return np.repeat(ids, triangle_counts), np.repeat(rc, triangle_counts, axis=0)


def write_vtk_polydata(model: SurfaceModel, path: str, colors=None) -> None:
    """``model`` as a legacy-VTK binary PolyData file: POINTS, POLYGONS, and per triangle SCALARS label (the smallest label
    id of its region) and COLOR_SCALARS colors (RGBA bytes).  ``colors``: a table as ``read_color_table`` gives it, uint8
    [n_regions, 4], or None for the fallback rule."""
    t = len(model.triangles)
    labels, rgba = _cell_data(model.regions, np.diff(model.triangle_offsets), colors)
    cells = np.concatenate([np.full((t, 1), 3, np.int32), model.triangles.astype(np.int32)], 1)
    _vtk_file(str(path), len(model.points), t, model.points.astype('>f4').tobytes(), cells.astype('>i4').tobytes(), labels, rgba)


def read_vtk_polydata(path: str) -> dict:
    """What ``write_vtk_polydata`` wrote -> {'title', 'points' float32 [n, 3], 'triangles' int32 [m, 3], 'labels' uint16 [m],
    'colors' uint8 [m, 4]}; anything else raises ValueError."""
    blob = open(path, 'rb').read()
    at = 0

    def line() -> str:
        nonlocal at
        end = blob.find(b'\n', at)
        if end < 0:
            raise ValueError(f'{path}: truncated at byte {at}')
        text, at = blob[at:end].decode('ascii'), end + 1
        return text

    def expect(text: str) -> None:
        got = line()
        if got != text:
            raise ValueError(f'{path}: expected {text!r}, found {got!r}')

    def block(dtype: str, count: int) -> np.ndarray:
        nonlocal at
        size = np.dtype(dtype).itemsize * count
        if at + size + 1 > len(blob) or blob[at + size:at + size + 1] != b'\n':
            raise ValueError(f'{path}: a section of {size} bytes at byte {at} does not end with a newline')
        arr, at = np.frombuffer(blob, dtype, count, at), at + size + 1
        return arr

    expect('# vtk DataFile Version 3.0')
    title = line()
    expect('BINARY')
    expect('DATASET POLYDATA')
    head = line().split()
    if len(head) != 3 or head[0] != 'POINTS' or head[2] != 'float':
        raise ValueError(f'{path}: not a POINTS n float line: {head}')
    n = int(head[1])
    points = block('>f4', 3 * n).astype(np.float32).reshape(n, 3)
    head = line().split()
    if len(head) != 3 or head[0] != 'POLYGONS' or int(head[2]) != 4 * int(head[1]):
        raise ValueError(f'{path}: not a POLYGONS m 4m line: {head}')
    t = int(head[1])
    cells = block('>i4', 4 * t).astype(np.int32).reshape(t, 4)
    if t and not np.all(cells[:, 0] == 3):
        raise ValueError(f'{path}: a polygon that is no triangle')
    expect(f'CELL_DATA {t}')
    expect('SCALARS label unsigned_short 1')
    expect('LOOKUP_TABLE default')
    labels = block('>u2', t).astype(np.uint16)
    expect('COLOR_SCALARS colors 4')
    colors = block('u1', 4 * t).reshape(t, 4).copy()
    if at != len(blob):
        raise ValueError(f'{path}: {len(blob) - at} bytes after the last section')
    return {'title': title, 'points': points, 'triangles': np.ascontiguousarray(cells[:, 1:]), 'labels': labels, 'colors': colors}


class VTKModelGenerator:
    """The reference's generator: ``VTKModelGenerator(color_file_path).generate_vtk_model(mask_path, output_path, ...)`` turns
    a label file into a coloured legacy-VTK PolyData model, one surface per label present."""

    def __init__(self, color_file_path: Optional[str] = None, device=None, decimation: bool = False):
        """``decimation=True``: honour ``decimation_factor`` in [0, 1) (the model is decimated on the device before it is
        downloaded); the default refuses a factor other than 0, as before decimation was built."""
        self.colors = read_color_table(color_file_path) if color_file_path is not None else None
        self.device = device
        self.decimation = bool(decimation)

    def _check(self, smoothing_factor, decimation_factor) -> Tuple[int, float]:
        if self.decimation:
            d = check_decimation(decimation_factor)
        elif decimation_factor != 0:
            raise NotImplementedError(f'decimation_factor={decimation_factor}: this generator was not made to decimate, make it with '
                                      f'VTKModelGenerator(..., decimation=True) or pass decimation_factor=0 (the reference passes 0.2)')
        else:
            d = 0.0
        return smoothing_pairs(smoothing_factor), d

    def _write(self, seg, affine, output_path: str, pairs_d: Tuple[int, float], coordinate_system: str) -> str:
        a = _check_affine(affine, None, coordinate_system)
        m = _device_mesh(seg, None, a, pairs_d[0], 1, self.device, decimation=pairs_d[1])
        points, cells, _ = m.payload()                              # the file's POINTS and POLYGONS bytes as the device stored them
        labels, rgba = _cell_data(m.regions, m.triangle_counts, self.colors)
        _vtk_file(str(output_path), m.n, m.t, points, cells, labels, rgba)
        return output_path

    def generate_vtk_model(self, mask_path: str, output_path: str, smoothing_factor: float = 0.5, decimation_factor: float = 0.0,
                           coordinate_system: str = 'RAS') -> str:
        """The label file ``mask_path`` (NIfTI) -> the model file ``output_path``; returns ``output_path``.  The map is decoded
        on the device in the file's frame and meshed with the header's affine."""
        from .imageio import NiftiIO, _affine_of
        pairs = self._check(smoothing_factor, decimation_factor)
        if coordinate_system not in ('RAS', 'LPS'):
            raise ValueError(f"coordinate_system must be 'RAS' or 'LPS', got {coordinate_system!r}")
        dev = torch.device(self.device) if self.device is not None else _device()
        with torch.cuda.device(dev):
            seg, properties = NiftiIO().read_label_map(str(mask_path))
            return self._write(seg, _affine_of(properties), output_path, pairs, coordinate_system)

    def generate_from_labels(self, seg, properties: dict, output_path: str, smoothing_factor: float = 0.5,
                             decimation_factor: float = 0.0, coordinate_system: str = 'RAS') -> str:
        """The same for a label map (z, y, x) that is still on the device after a prediction; the affine comes from the
        case's properties as the label writer takes it."""
        from .imageio import _affine_of
        pairs = self._check(smoothing_factor, decimation_factor)
        return self._write(seg, _affine_of(properties), output_path, pairs, coordinate_system)
