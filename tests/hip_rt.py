"""Device buffers and streams through the HIP runtime libgdpt.so itself has loaded (found in this process's maps), for tests of the
device-pointer entry points that stay in the suite's process. Not collected by pytest."""
import ctypes as C

import numpy as np

_rt = None


def rt(G):
    global _rt
    if _rt is None:
        G.lib()
        path = next(l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l)
        _rt = C.CDLL(path)
    return _rt


def ck(rc):
    assert rc == 0, f"HIP runtime call failed: {rc}"


def alloc(G, nbytes):
    p = C.c_void_p()
    ck(rt(G).hipMalloc(C.byref(p), C.c_size_t(nbytes)))
    return p.value


def upload(G, a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    p = alloc(G, a.nbytes)
    ck(rt(G).hipMemcpy(C.c_void_p(p), C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1))      # hipMemcpyHostToDevice
    return p


def to_host(G, ptr, shape):
    out = np.empty(shape, dtype=np.float64)
    ck(rt(G).hipDeviceSynchronize())
    ck(rt(G).hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2))      # hipMemcpyDeviceToHost
    return out


def free(G, ptr):
    ck(rt(G).hipFree(C.c_void_p(ptr)))


def stream(G):
    s = C.c_void_p()
    ck(rt(G).hipStreamCreate(C.byref(s)))
    return s.value


def stream_destroy(G, s):
    ck(rt(G).hipStreamDestroy(C.c_void_p(s)))
