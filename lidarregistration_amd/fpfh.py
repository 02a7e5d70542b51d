"""FPFH descriptors on the GPU and their matching: the reference's other descriptor (Experiments/demo_registration.py:37-44 and
--descriptor fpfh, datasets/KITTI.py:51-53,85-93, misc/cal_fpfh.py:22-26), for users without trained FCGF weights.  lr_fpfh
(csrc/lr_fpfh.hip) computes the 33-number histograms under the contract F1..F6 of include/lidarreg.h (Open3D's
compute_fpfh_feature is not vendored, its algorithm is upstream-recalled); the 33-wide rows are matched by lr_nn_wide through
matching.find_nn.  No CPU fallback.

Not built: the demo's order (normals estimated on the raw cloud and averaged by the down-sampling; here, as misc/cal_fpfh.py does, they
are estimated on the down-sampled cloud), and several clouds per call.
"""
import torch

from . import _ext, devmem, matching
from .bbrf import normals_dev
from .devmem import f64, ptr
from .matching import _device, _stream
from .overlap import voxel_down_sample

DIM = 33


def fpfh_dev(xyz, normals, radius, max_nn=100, want_f64=True, want_f32=True, poison=None):
    """lr_fpfh of xyz, normals [n,3] (float64).  Returns (F64 [n,33] float64 or None, F32 [n,33] float32 or None -- device tensors --,
    dict(status, dropped, zero_rows, capped))."""
    dev = _device()
    x, nr = f64(xyz, dev), f64(normals, dev)
    n = int(x.shape[0])
    assert nr.shape[0] == n, "one normal per point"
    L = _ext.lib()
    o64 = torch.empty((max(n, 1), DIM), dtype=torch.float64, device=dev) if want_f64 else None
    o32 = torch.empty((max(n, 1), DIM), dtype=torch.float32, device=dev) if want_f32 else None
    info = torch.empty(4, dtype=torch.int32, device=dev)
    need = L.lr_fpfh_scratch_bytes(n, int(max_nn))
    scratch = devmem.scratch(need, dev, poison)
    _ext.check(L.lr_fpfh(ptr(x, n), ptr(nr, n), n, float(radius), int(max_nn), ptr(o64), ptr(o32), info.data_ptr(),
                         scratch.data_ptr(), scratch.numel(), _stream()))
    status, dropped, zero_rows, capped = (int(v) for v in info.cpu())
    return (None if o64 is None else o64[:n], None if o32 is None else o32[:n],
            dict(status=status, dropped=dropped, zero_rows=zero_rows, capped=capped))


def compute_fpfh(xyz, normals, radius, max_nn=100):
    """Open3D's compute_fpfh_feature(pcd, KDTreeSearchParamHybrid(radius, max_nn)) as an [n,33] float64 numpy array (``fpfh.data.T``)."""
    return fpfh_dev(xyz, normals, radius, max_nn, want_f32=False)[0].cpu().numpy()


def extract(raw_xyz, voxel_size):
    """misc/cal_fpfh.py:22-26: voxel down-sampling, normals with the hybrid search (radius 2 voxel, 30 neighbours), FPFH with (radius
    5 voxel, 100 neighbours).  Returns (points [n,3] float64, features [n,33] float32) as device tensors."""
    v = float(voxel_size)
    pts = voxel_down_sample(raw_xyz, v)
    nrm, _ = normals_dev(pts, radius=2.0 * v, max_nn=30)
    _, F, _ = fpfh_dev(pts, nrm, 5.0 * v, 100, want_f64=False)
    return pts, F


class Extractor:
    """extract() behind the interface harness.RefCloudSource(extractor=...) takes (the CLI's --descriptor fpfh): the raw scan
    down-sampled, its 33-number rows normalised as datasets/KITTI.py:52-53 does before matching.  One cloud per call."""

    def __init__(self, voxel_size=0.3):
        self.voxel_size = float(voxel_size)

    def extract(self, raw, voxel_size=None):
        """(xyz [n,3] float32, feats [n,33] float32, info) -- device tensors -- of one raw scan [N,3]."""
        v = self.voxel_size if voxel_size is None else float(voxel_size)
        pts, F = extract(raw, v)
        return pts.to(torch.float32), normalise(F).contiguous(), dict(n=int(pts.shape[0]), voxel_size=v)

    def extract_batch(self, raws, voxel_size=None):
        """extract() of every scan in turn (lr_fpfh takes one cloud per call)."""
        return [self.extract(raw, voxel_size) for raw in raws]


def normalise(F):
    """datasets/KITTI.py:52-53: every row divided by (its L2 norm + 1e-6), float32 in and out (torch tensor, on the device it is on)."""
    F = torch.as_tensor(F).to(torch.float32)
    return F / (torch.linalg.norm(F, dim=1, keepdim=True) + 1e-6)


def mutual_pairs(idx01, idx10):
    """datasets/KITTI.py:85-93: the pairs (i, idx01[i]) -- with mutual only those whose target points back, idx10[idx01[i]] == i -- in
    ascending i, as an [m,2] int64 tensor."""
    idx01 = torch.as_tensor(idx01).long().cpu(); idx10 = torch.as_tensor(idx10).long().cpu()
    i = torch.arange(idx01.shape[0])
    keep = (idx01 >= 0) & (idx10[idx01.clamp(min=0)] == i) if idx10.shape[0] else torch.zeros_like(i, dtype=torch.bool)
    return torch.stack([i[keep], idx01[keep]], dim=1)


def match(F0, F1, mutual=True):
    """datasets/KITTI.py:52-53,85-93: the rows normalised, the nearest neighbour of every row of F0 among F1 (matching.find_nn: lr_nn_wide
    at 33 numbers) and, with mutual, the other way; returns corr [m,2] int64 (CPU tensor)."""
    dev = _device()
    A, B = normalise(torch.as_tensor(F0).to(dev)), normalise(torch.as_tensor(F1).to(dev))
    _, i01, _ = matching.find_nn(A, B)
    if not mutual:
        return torch.stack([torch.arange(i01.shape[0]), i01], dim=1)
    _, i10, _ = matching.find_nn(B, A)
    return mutual_pairs(i01, i10)
