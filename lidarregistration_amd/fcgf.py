"""FCGF descriptors on top of liblidarreg.so: lr_fcgf_extract (csrc/lr_fcgf.hip) runs the reference's feature network --
``ResUNetBN2C(1, 32, conv1_kernel_size=5, normalize_feature=True)`` of Experiments/misc/fcgf.py, which the reference evaluates on
MinkowskiEngine for every pair (Experiments/datasets/LidarFeatureExtractor.py:71-81, :166-181) -- on integer voxel cells.  This module
packs the reference's checkpoint (``torch.load(file)['state_dict']``) into the library's weight blob and wraps the call.  The contract is
n1 of include/lidarreg.h, restated in numpy in tests/fcgf_cpu.py.  lr_fcgf_extract_batch (contract n2, §18.7) takes up
to 64 clouds per call and gives every cloud the bytes of the one-cloud call: features_batch, extract_batch, extract_pairs.  There is no
CPU fallback.
"""
import ctypes

import numpy as np
import torch

from . import _ext, devmem, resunet
from .devmem import ptr

N_STAGES = resunet.N_STAGES
MAX_N = 1 << 20
MAX_CLOUDS = 64            # clouds per lr_fcgf_extract_batch (MAX_N rows together)
WIDTHS = (32, 64, 128, 256, 128, 64, 64, 64)          # ResUNetBN2C: C1 C2 C3 C4 (down), T4 T3 T2 T1 (up)


def stage_plan(conv1_kernel_size=5):
    """The 23 stages in order: (conv module, norm module | None, K^3, Cin, Cout) -- the module names of fcgf.py:644-798."""
    if conv1_kernel_size not in (3, 5):
        raise ValueError(f"conv1_kernel_size must be 3 or 5, not {conv1_kernel_size!r}")
    return resunet.stage_plan(WIDTHS, conv1_kernel_size ** 3, 27, 32)


def packed_floats(conv1_kernel_size=5):
    return resunet.packed_floats(stage_plan(conv1_kernel_size))


def fold(sd, conv1_kernel_size=5, dtype=np.float32):
    """[(W [K^3,Cin,Cout], scale [Cout], offset [Cout])] per stage, as `dtype`: BatchNorm folded in fp64 and rounded once (float64: not at
    all -- what tests/fcgf_cpu.py's fp64 restatement evaluates).  A 1x1 kernel may be [Cin,Cout] or [1,Cin,Cout]; a missing key, a wrong
    shape or a non-finite value is a ValueError naming the key."""
    return resunet.fold(sd, stage_plan(conv1_kernel_size), "FCGF state dict", False, dtype)


def pack(sd, conv1_kernel_size=5):
    """The flat float32 blob of lr_fcgf_weights_bytes(conv1_kernel_size) bytes: per stage W, scale, offset."""
    return resunet.pack(fold(sd, conv1_kernel_size))


def unpack(blob, conv1_kernel_size=5):
    """pack() undone: the stages of a blob."""
    return resunet.unpack(blob, stage_plan(conv1_kernel_size))


class FCGF:
    """The feature network with one set of weights on one device."""

    def __init__(self, blob, conv1_kernel_size=5, device=None):
        L = _ext.lib()
        self.conv1_kernel_size = int(conv1_kernel_size)
        blob = np.ascontiguousarray(blob, np.float32).reshape(-1)
        want = L.lr_fcgf_weights_bytes(self.conv1_kernel_size)
        if want == 0 or blob.nbytes != want:
            raise ValueError(f"weight blob of {blob.nbytes} bytes, lr_fcgf_weights_bytes({self.conv1_kernel_size}) = {want}")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.weights = torch.from_numpy(blob).to(self.device)
        self.last_info = None

    @classmethod
    def from_state_dict(cls, sd, conv1_kernel_size=5, device=None):
        """sd: the reference's state dict (tensors or arrays): <conv>.kernel, final.bias and <norm>.bn.{weight,bias,running_mean,
        running_var}; other keys (num_batches_tracked) are ignored."""
        return cls(pack(sd, conv1_kernel_size), conv1_kernel_size, device)

    @classmethod
    def from_checkpoint(cls, path, conv1_kernel_size=None, device=None):
        """The reference's checkpoint file (LidarFeatureExtractor.py:79-80): torch.load(path)['state_dict'].  conv1_kernel_size: read from
        conv1.kernel's shape unless given."""
        ck = torch.load(path, map_location="cpu")
        sd = ck["state_dict"] if isinstance(ck, dict) and "state_dict" in ck else ck
        if conv1_kernel_size is None:
            k3 = int(resunet.np64(sd, "conv1.kernel", None, "FCGF state dict").shape[0])
            conv1_kernel_size = {27: 3, 125: 5}.get(k3)
            if conv1_kernel_size is None:
                raise ValueError(f"FCGF state dict: conv1.kernel has {k3} offsets, expected 27 or 125")
        return cls.from_state_dict(sd, conv1_kernel_size, device)

    def _call(self, coords, feat_in, tap, poison=None):
        L = _ext.lib()
        dev = self.device
        coords = torch.as_tensor(coords).to(device=dev, dtype=torch.int32).contiguous().reshape(-1, 3)
        n = int(coords.shape[0])
        if feat_in is not None:
            feat_in = torch.as_tensor(feat_in).to(device=dev, dtype=torch.float32).contiguous().reshape(-1)
            if feat_in.shape[0] != n:
                raise ValueError(f"feat_in has {feat_in.shape[0]} rows, coords {n}")
        scratch = devmem.scratch(L.lr_fcgf_scratch_bytes(n), dev, poison)
        res = torch.zeros(ctypes.sizeof(_ext.FcgfResult), dtype=torch.uint8, device=dev)
        out = torch.zeros((max(n, 1), 256 if tap else 32), dtype=torch.float32, device=dev)
        tc = torch.zeros((max(n, 1), 3), dtype=torch.int32, device=dev) if tap else None
        params = _ext.FcgfParams(conv1_kernel_size=self.conv1_kernel_size, tap=int(tap))
        with torch.cuda.device(dev):
            _ext.check(L.lr_fcgf_extract(ptr(coords, n), ptr(feat_in, n), n, self.weights.data_ptr(), self.weights.numel() * 4, ctypes.byref(params),
                                         res.data_ptr(), ptr(out, n), ptr(tc, n), scratch.data_ptr(), scratch.numel(), torch.cuda.current_stream().cuda_stream))
        return n, out, tc, res

    def features(self, coords, feat_in=None, poison=None):
        """coords [n,3] integer voxel cells (distinct), feat_in [n] or None = ones -> [n,32] float32 device tensor, row i for cell i.
        self.last_info: the result block (status 2: a duplicate cell, 3: a cell past the range limit; the rows are 0 then).
        poison: fill the scratch with this byte first (test hook)."""
        n, out, _, res = self._call(coords, feat_in, 0, poison)
        r = devmem.read_struct(res, _ext.FcgfResult)
        self.last_info = dict(status=r.status, n=r.n, n_tap=r.n_tap)
        return out[:n]

    def tap(self, coords, s, feat_in=None):
        """Stage s (1..23) alone: (activations [n_level, Cout], the level's cells [n_level, 3]) as device tensors."""
        if not 1 <= int(s) <= N_STAGES:
            raise ValueError(f"tap stage must lie in 1..{N_STAGES}")
        n, out, tc, res = self._call(coords, feat_in, int(s))
        r = devmem.read_struct(res, _ext.FcgfResult)
        self.last_info = dict(status=r.status, n=r.n, n_tap=r.n_tap)
        cout = stage_plan(self.conv1_kernel_size)[int(s) - 1][4]
        return out.reshape(-1)[:r.n_tap * cout].reshape(r.n_tap, cout), tc[:r.n_tap]

    def _call_batch(self, coords, feat_in, poison=None):
        """One lr_fcgf_extract_batch over device tensors coords[b] [n_b,3] int32 and feat_in[b] [n_b] float32 | None (at most MAX_CLOUDS
        clouds and MAX_N rows together) -> (outs [n_b,32], the result blocks as one uint8 tensor)."""
        L = _ext.lib()
        dev = self.device
        B = len(coords)
        ns = [int(c.shape[0]) for c in coords]
        outs = [torch.zeros((max(n, 1), 32), dtype=torch.float32, device=dev) for n in ns]
        res = torch.zeros(B * ctypes.sizeof(_ext.FcgfResult), dtype=torch.uint8, device=dev)
        scratch = devmem.scratch(L.lr_fcgf_batch_scratch_bytes(B, sum(ns)), dev, poison)
        arr = lambda ts: (ctypes.c_void_p * B)(*[ptr(t, n) for t, n in zip(ts, ns)])
        params = _ext.FcgfParams(conv1_kernel_size=self.conv1_kernel_size, tap=0)
        with torch.cuda.device(dev):
            _ext.check(L.lr_fcgf_extract_batch(B, arr(coords), arr(feat_in), (ctypes.c_int32 * B)(*ns), self.weights.data_ptr(), self.weights.numel() * 4,
                                               ctypes.byref(params), res.data_ptr(), arr(outs), scratch.data_ptr(), scratch.numel(),
                                               torch.cuda.current_stream().cuda_stream))
        return [o[:n] for o, n in zip(outs, ns)], res

    def features_batch(self, cells_list, feat_in_list=None, poison=None):
        """`features` for many clouds through lr_fcgf_extract_batch (contract n2): cells_list[b] [n_b,3], feat_in_list[b] [n_b] or None = ones
        -> a list of [n_b,32] device tensors, each holding the bytes `features` gives for that cloud alone.  self.last_info: one dict per
        cloud; the status is per cloud (3: a cell past +-(2^18 - 2), the batch entry's range).  Lists of more than MAX_CLOUDS clouds or
        MAX_N rows are split into several calls; a single cloud above MAX_N rows is refused by the library."""
        dev = self.device
        coords = [torch.as_tensor(c).to(device=dev, dtype=torch.int32).contiguous().reshape(-1, 3) for c in cells_list]
        feat_in = list(feat_in_list) if feat_in_list is not None else [None] * len(coords)
        if len(feat_in) != len(coords):
            raise ValueError(f"feat_in_list has {len(feat_in)} entries, cells_list {len(coords)}")
        for b, f in enumerate(feat_in):
            if f is not None:
                feat_in[b] = f = torch.as_tensor(f).to(device=dev, dtype=torch.float32).contiguous().reshape(-1)
                if f.shape[0] != coords[b].shape[0]:
                    raise ValueError(f"feat_in_list[{b}] has {f.shape[0]} rows, cells_list[{b}] {coords[b].shape[0]}")
        outs, blocks = [], []
        at = 0
        while at < len(coords):
            end, rows = at + 1, int(coords[at].shape[0])
            while end < len(coords) and end - at < MAX_CLOUDS and rows + int(coords[end].shape[0]) <= MAX_N:
                rows += int(coords[end].shape[0]); end += 1
            o, res = self._call_batch(coords[at:end], feat_in[at:end], poison)
            outs += o; blocks.append(res)
            at = end
        self.last_info = []
        for res in blocks:
            host = res.cpu()
            for k in range(host.numel() // ctypes.sizeof(_ext.FcgfResult)):
                r = devmem.read_struct(host, _ext.FcgfResult, k)
                self.last_info.append(dict(status=r.status, n=r.n, n_tap=r.n_tap))
        return outs

    def extract_batch(self, raw_scans, voxel_size=0.3):
        """`extract` for many raw scans: [(xyz_kept, feats, sel)] in their order, the voxel de-duplication per cloud and the network in one
        batched call.  A cloud with a non-zero status raises, naming its index."""
        from . import voxel
        kept, cells = [], []
        with torch.cuda.device(self.device):
            for raw in raw_scans:
                xyz, sel = voxel.voxel_downsample(raw, voxel_size)
                x64 = torch.as_tensor(raw).to(device=self.device, dtype=torch.float64)[sel]
                kept.append((xyz, sel)); cells.append(torch.floor(x64 / voxel_size).to(torch.int32))
            feats = self.features_batch(cells)
        for b, info in enumerate(self.last_info):
            if info["status"] != 0:
                raise _ext.LidarRegError(f"lr_fcgf_extract_batch: cloud {b}: status {info['status']} (2: duplicate cell, 3: cell past the range limit of 2^18 - 2)")
        return [(xyz, f, sel) for (xyz, sel), f in zip(kept, feats)]

    def extract_pairs(self, pairs, voxel_size=0.3):
        """[(xyz0_raw, xyz1_raw)] -> [(xyz0, xyz1, feats0, feats1)], `extract_pair` for every pair with both clouds of every pair in one
        batched call, as the reference batches a pair into one sparse tensor (LidarFeatureExtractor.py:166-181)."""
        out = self.extract_batch([raw for pair in pairs for raw in pair], voxel_size)
        return [(out[2 * k][0], out[2 * k + 1][0], out[2 * k][1], out[2 * k + 1][1]) for k in range(len(pairs))]

    def extract(self, xyz_raw, voxel_size=0.3):
        """A raw scan [N,3] -> (xyz_kept [n,3] float32, feats [n,32], sel [n] int64), device tensors: the reference's loader
        (generic_balanced_loader.py:62-66, :81: voxel de-duplication, floor(xyz / voxel_size), features of ones) and its network."""
        from . import voxel
        with torch.cuda.device(self.device):
            xyz, sel = voxel.voxel_downsample(xyz_raw, voxel_size)
            x64 = torch.as_tensor(xyz_raw).to(device=self.device, dtype=torch.float64)[sel]
            cells = torch.floor(x64 / voxel_size).to(torch.int32)
            feats = self.features(cells)
        if self.last_info["status"] != 0:
            raise _ext.LidarRegError(f"lr_fcgf_extract: status {self.last_info['status']} (2: duplicate cell, 3: cell past the range limit of 2^20 - 2)")
        return xyz, feats, sel

    def extract_pair(self, xyz0_raw, xyz1_raw, voxel_size=0.3):
        """Two raw scans -> (xyz0, xyz1, feats0, feats1), the arguments of FR() in its order: what LidarFeatureExtractor.process_batch
        computes for one pair."""
        xyz0, f0, _ = self.extract(xyz0_raw, voxel_size)
        xyz1, f1, _ = self.extract(xyz1_raw, voxel_size)
        return xyz0, xyz1, f0, f1
