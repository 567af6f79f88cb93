"""What the GPU tests of the kappa routes share (test_gpu_kappa.py, test_gpu_stretched.py, test_gpu_periodic.py): a device
array without PyTorch, the resident runs of a hierarchy and their comparison, mgSolve's parameters and the comparison of
two solves.  Not a test module; the worker scripts those files start in a fresh process keep their own copies."""
import ctypes

import numpy as np

import kappa_cases as kc


class DeviceArray:
    """A NumPy array's copy in HBM with __cuda_array_interface__ (hipMalloc / hipMemcpy / hipFree through the HIP runtime
    the library itself uses: no PyTorch in this process)."""
    hip = None

    def __init__(self, host):
        if DeviceArray.hip is None:
            hip = ctypes.CDLL("libamdhip64.so.7")
            hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
            hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
            hip.hipFree.argtypes = [ctypes.c_void_p]
            DeviceArray.hip = hip
        host = np.ascontiguousarray(host)
        self.shape, self.dtype, self.nbytes = host.shape, host.dtype, host.nbytes
        self.d = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(self.d), max(host.nbytes, 8)) == 0
        assert self.hip.hipMemcpy(self.d, host.ctypes.data, host.nbytes, 1) == 0

    @property
    def __cuda_array_interface__(self):
        return {"shape": tuple(self.shape), "typestr": self.dtype.str, "data": (self.d.value, False), "version": 2, "strides": None}

    def numpy(self):
        out = np.empty(self.shape, dtype=self.dtype)
        assert self.hip.hipMemcpy(out.ctypes.data, self.d, self.nbytes, 2) == 0
        return out

    def __del__(self):
        if self.d:
            self.hip.hipFree(self.d)
            self.d = None


def run(h, b, x0, cycles):
    h.resident_load(b, x0)
    return [h.resident_cycle(1, 1) for _ in range(cycles)], h.resident_fetch()


def run_pcg(h, b, x0, iterations):
    h.resident_load(b, x0)
    it, norms, true_norm, breakdown = h.resident_pcg(1, 1, iterations)
    return [it, true_norm, breakdown] + list(norms), h.resident_fetch()


def same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1])


def flags(h):
    return [h.level_flags(l) for l in range(h.n_levels - 1)]


def vectors(shape, dtype="float64"):
    b, x0 = kc.rhs_of(shape)
    if dtype != "float64":
        b, x0 = b.astype(np.float32).astype(np.float64), x0.astype(np.float32).astype(np.float64)
    return b, x0


def params(shape, grids, cycles, **more):
    return dict({"problemShape": shape, "gridLevels": grids, "preIterations": 1, "postIterations": 1, "smoother": "colour",
                 "cycles": cycles, "threshold": 0.0, "minSize": 8}, **more)


def same_solve(a, b):
    return np.array_equal(a[0], b[0]) and a[1]["norms"] == b[1]["norms"] and a[1]["cycle"] == b[1]["cycle"] and a[1]["norm"] == b[1]["norm"]
