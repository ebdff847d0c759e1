"""What the plan-level GPU tests (tests/test_sphnet_units_gpu.py, tests/test_iresnet_units_gpu.py) share to drive a plan through the raw C ABI on
their own buffers: guarded byte buffers, the finite sentinels, the profile counters per slot and the plan's inventories (fedfr_net_query,
fedfr_net_tensor_info, fedfr_net_act_info).  No test lives here."""
import ctypes as C

import torch

from fedfr_amd import _C

GUARD = 1 << 16                                             # bytes
GUARD_BYTE = 0xA5
SENTINELS = (30000.0, -12345.0)                             # finite in fp16 and bf16, and as the fp32 two such 16-bit patterns spell
CUS = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
SLOTS = range(27)


def dev():
    return torch.device("cuda:0")


def slot_counts():
    out = {}
    for s in SLOTS:
        ms, n, fl = C.c_double(0), C.c_longlong(0), C.c_double(0)
        _C.call("fedfr_profile_read", s, C.byref(ms), C.byref(n), C.byref(fl))
        if n.value:
            out[s] = n.value
    return out


class Guarded:
    """a byte buffer with a guard band behind it"""

    def __init__(self, nbytes):
        self.n = (nbytes + 15) // 16 * 16
        self.buf = torch.empty(self.n + GUARD, dtype=torch.uint8, device=dev())
        self.buf[self.n:] = GUARD_BYTE

    def view(self, dtype):
        return self.buf[:self.n].view(dtype)

    def ptr(self):
        return self.buf.data_ptr()

    def guard_ok(self):
        return bool((self.buf[self.n:] == GUARD_BYTE).all())


def query(h, key):
    q = C.c_longlong()
    _C.call("fedfr_net_query", h, key, C.byref(q))
    return q.value


def tensor_table(h):
    out = []
    for i in range(query(h, _C.Q_NUM_TENSORS)):
        name, kind, region, off, ndim, shape = C.create_string_buffer(128), C.c_int(), C.c_int(), C.c_longlong(), C.c_int(), (C.c_int * 4)()
        _C.call("fedfr_net_tensor_info", h, i, name, 128, C.byref(kind), C.byref(region), C.byref(off), C.byref(ndim), shape)
        out.append((name.value.decode(), tuple(shape[:ndim.value]), off.value, region.value))
    return out


def act_info(h, block, which):
    off, rows, ch = C.c_longlong(), C.c_int(), C.c_int()
    _C.call("fedfr_net_act_info", h, block, which, C.byref(off), C.byref(rows), C.byref(ch))
    return off.value, rows.value, ch.value
