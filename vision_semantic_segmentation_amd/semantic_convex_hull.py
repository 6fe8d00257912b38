"""Semantic extraction: the convex hulls of a class's largest connected regions (src/semantic_convex_hull.py:17-91) on the GPU.

``generate_convex_hull`` keeps the reference's signature and return value.  ``label_components_device`` and
``class_hulls_device`` are the device forms: several label maps and several classes in one call (csrc/seg_hull.hip), results left on
the device; ``ClassHulls.host()`` brings every hull of a call to the host in ONE copy.
"""
import collections
import ctypes as C

import numpy as np
import torch

from . import _lib

MAX_TOP_NUMBER = 8


def _maps(maps):
    """ndarray / tensor [h, w] or [N, h, w] -> (contiguous CUDA uint8 [N, h, w], batched?)"""
    t = maps if isinstance(maps, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(maps))
    if t.dim() not in (2, 3):
        raise ValueError("a label map is [h, w] or [N, h, w], got shape %s" % (tuple(t.shape),))
    if t.dtype != torch.uint8:
        if t.is_floating_point() or bool(((t < 0) | (t > 255)).any()):
            raise ValueError("label maps hold class ids 0 .. 255 (uint8), got dtype %s" % (t.dtype,))
        t = t.to(torch.uint8)
    t = t.cuda() if not t.is_cuda else t
    batched = t.dim() == 3
    return (t if batched else t[None]).contiguous(), batched


def _classes(classes):
    cl = [int(c) for c in (classes if isinstance(classes, (list, tuple, np.ndarray)) else [classes])]
    if not cl:
        raise ValueError("no class index given")
    return cl, (C.c_int32 * len(cl))(*cl)


def _stream(t, stream):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream if stream is None else stream)


def label_components_device(maps, classes, erode=True, stream=None):
    """Connected components (8-connectivity) of (map == class) for every map and class: semantic_convex_hull.py:36-51 up to the
    numbering.  maps [h, w] or [N, h, w]; returns CUDA int32 [len(classes), h, w] or [N, len(classes), h, w]: 0 = background,
    otherwise 1 + the smallest linear index y * w + x of the component.  erode=False skips the 3x3 erosion."""
    t, batched = _maps(maps)
    cl, cl_host = _classes(classes)
    n, h, w = (int(v) for v in t.shape)
    out = torch.empty((n, len(cl), h, w), dtype=torch.int32, device=t.device)
    _lib.check(_lib.lib().avl_label_components(C.c_void_p(t.data_ptr()), n, h, w, cl_host, len(cl), int(bool(erode)),
                                               C.c_void_p(out.data_ptr()), None, _stream(t, stream)), "avl_label_components")
    return out if batched else out[0]


class ClassHulls(collections.namedtuple("ClassHulls", "vertices n_vertices areas roots packed")):
    """What class_hulls_device returns, CUDA int32 tensors with leading dimensions [len(classes), top_number] (or
    [N, len(classes), top_number]): vertices [..., 2h+1, 2] as (x, y), n_vertices, areas, roots (include/avl_hip.h).  All four
    are views of ``packed``, so one copy moves them together."""
    __slots__ = ()

    def host(self):
        """One device-to-host copy -> ClassHulls of ndarrays."""
        flat = self.packed.cpu().numpy()
        lead, nv = tuple(self.n_vertices.shape), self.vertices.numel()
        cnt = self.n_vertices.numel()
        return ClassHulls(flat[:nv].reshape(tuple(self.vertices.shape)), flat[nv:nv + cnt].reshape(lead),
                          flat[nv + cnt:nv + 2 * cnt].reshape(lead), flat[nv + 2 * cnt:nv + 3 * cnt].reshape(lead), flat)

    def polygons(self):
        """Per leading index but the last (class, or image and class): the list the reference returns for that class -- one int32
        array [2, n + 1] per hull, closed by repeating the first vertex (:75), slots without vertices left out.  Nested lists."""
        hst = self if isinstance(self.packed, np.ndarray) else self.host()

        def walk(v, n):
            if n.ndim == 1:
                return [np.concatenate([v[k, :n[k]], v[k, :1]], axis=0).T.astype(np.int32) for k in range(n.shape[0]) if n[k] > 0]
            return [walk(v[i], n[i]) for i in range(n.shape[0])]
        return walk(hst.vertices, hst.n_vertices)


def hull_workspace_bytes(h, w, planes, top_number=1):
    return int(_lib.lib().avl_hull_scratch_bytes(int(h), int(w), int(planes), int(top_number)))


def class_hulls_device(maps, classes, top_number=1, area_threshold=30, drop_first=True, workspace=None, stream=None, erode=True):
    """semantic_convex_hull.py:36-76 for every map and class in ONE call: erosion, components, the top_number largest with more than
    area_threshold pixels, their convex hulls.  workspace: a CUDA uint8 tensor of at least hull_workspace_bytes(...) bytes to reuse
    between frames (allocated per call when None).  Nothing is synchronised; returns ClassHulls of device tensors."""
    t, batched = _maps(maps)
    cl, cl_host = _classes(classes)
    n, h, w = (int(v) for v in t.shape)
    top = int(top_number)
    if not 1 <= top <= MAX_TOP_NUMBER:
        raise ValueError("top_number must be 1 .. %d, got %d" % (MAX_TOP_NUMBER, top))
    planes = n * len(cl)
    need = hull_workspace_bytes(h, w, planes, top)
    if workspace is None:
        workspace = torch.empty(max(need, 8), dtype=torch.uint8, device=t.device)
    elif not (workspace.is_cuda and workspace.dtype == torch.uint8 and workspace.is_contiguous() and workspace.numel() >= need):
        raise ValueError("workspace must be a contiguous CUDA uint8 tensor of at least %d bytes" % need)
    cap, slots = 2 * h + 1, planes * top
    packed = torch.empty(slots * cap * 2 + 3 * slots, dtype=torch.int32, device=t.device)
    nv = slots * cap * 2
    lead = (n, len(cl), top) if batched else (len(cl), top)
    vertices, n_vertices = packed[:nv].view(lead + (cap, 2)), packed[nv:nv + slots].view(lead)
    areas, roots = packed[nv + slots:nv + 2 * slots].view(lead), packed[nv + 2 * slots:].view(lead)
    rc = _lib.lib().avl_class_hulls(C.c_void_p(t.data_ptr()), n, h, w, cl_host, len(cl), int(bool(erode)), top, int(area_threshold),
                                    int(bool(drop_first)), C.c_void_p(vertices.data_ptr()), C.c_void_p(n_vertices.data_ptr()),
                                    C.c_void_p(areas.data_ptr()), C.c_void_p(roots.data_ptr()), C.c_void_p(workspace.data_ptr()),
                                    _stream(t, stream))
    _lib.check(rc, "avl_class_hulls")
    return ClassHulls(vertices, n_vertices, areas, roots, packed)


def generate_convex_hull(img_src, vis=False, index_care_about=1, index_to_vitualize=None, top_number=1, area_threshold=30):
    """The reference's function (:17-91).  img_src: label map [h, w], ndarray or CUDA uint8 tensor.  Returns a list of int32 arrays
    [2, n + 1] -- the hull's (x, y) vertices with the first repeated at the end (:75) -- for the top_number largest connected regions
    of class index_care_about that have more than area_threshold pixels after a 3x3 erosion; [] when nothing qualifies (:53-54).
    As in the reference, a region's raster-first pixel is not part of its hull (:71).  The plotting options are not built."""
    if index_care_about == 0:
        raise ValueError("index care about cannot be zero in this version of code")       # :33-35 logs this and exits
    if vis or index_to_vitualize is not None:
        raise NotImplementedError("generate_convex_hull: vis / index_to_vitualize (matplotlib figures) are not built")
    if getattr(img_src, "ndim", None) != 2 and not (isinstance(img_src, torch.Tensor) and img_src.dim() == 2):
        raise ValueError("generate_convex_hull takes one [h, w] label map")
    return class_hulls_device(img_src, [index_care_about], top_number=top_number, area_threshold=area_threshold).polygons()[0]
