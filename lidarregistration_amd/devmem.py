"""Device buffers around a C call with a caller-owned scratch: the inputs as the library reads them, the scratch, nullable pointers and
the read-back of a result struct.  The C side's counterpart is csrc/lr_scratch.h.
"""
import ctypes

import numpy as np
import torch


def f64(X, dev):
    return torch.as_tensor(X).to(device=dev, dtype=torch.float64).contiguous().reshape(-1, 3)


def T_dev(T, dev):
    return None if T is None else torch.as_tensor(np.ascontiguousarray(T, np.float64).reshape(16)).to(dev)


def scratch(nbytes, dev, poison=None):
    """256-byte aligned device scratch (torch's allocator aligns to 512) of at least 256 bytes.  poison: fill it with this byte first
    (test hook: no result depends on what a scratch holds)."""
    s = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)
    if poison is not None:
        s.fill_(int(poison))
    return s


def ptr(t, n=1):
    """The tensor's address, None for a missing tensor or an empty one (n rows)."""
    return None if t is None or not n else t.data_ptr()


def read_struct(buf, Struct, k=0):
    """Struct number k of the uint8 tensor buf: one device-to-host copy (it synchronises with the current stream); a caller that reads
    several structs passes buf.cpu() and copies once."""
    size = ctypes.sizeof(Struct)
    return Struct.from_buffer_copy(buf.reshape(-1)[k * size:(k + 1) * size].cpu().numpy().tobytes())


def as_dict(struct):
    """The struct's fields by name; arrays of doubles as numpy arrays, 16 of them as a 4x4 matrix."""
    out = {}
    for name, _ in struct._fields_:
        v = getattr(struct, name)
        if isinstance(v, ctypes.Array) and v._type_ is ctypes.c_double:
            v = np.array(v, np.float64)
            v = v.reshape(4, 4) if v.size == 16 else v
        out[name] = v
    return out
