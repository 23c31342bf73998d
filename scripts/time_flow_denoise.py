"""Timing record of the weighted flow denoiser (a record, not a gate):
writes profiles/flow_denoise_times.txt.

388 x 584 (the Dimetrodon ground-truth flow, unknowns zeroed), K = 9, 50
iterations, device arrays.  HIP events around each call after a 0.5 s warm-up;
per variant the median of five calls, the variants interleaved in one process
(round r times every variant once), and the spread (min .. max) beside it.

  parent   gqmap_cpu_run_device of another build of the library (--parent-lib:
           the parent commit's libgqmap.so; left out when not given)
  cpu_run  gqmap_cpu_run_device of this build
  ref      gqmap_flow_denoise_device, var = NULL, reference scatter: the same
           kernels as cpu_run plus the start's check, so expected within the
           rounds' spread
  field    gqmap_flow_denoise_device with a variance field, a start and the
           adjoint scatter
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: one HIP runtime in the process)

from gqmap_opticalflow_amd import _lib, flow_to_color, flowio  # noqa: E402
from gqmap_opticalflow_amd.legacy import _fortran_dev, cpu_options  # noqa: E402

ITS, ROUNDS, WARM_S = 50, 5, 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libgqmap.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_denoise_times.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.init()
    lib = _lib.load()
    gt = flowio.load_pair("Dimetrodon")[2]
    flo = np.asfortranarray(flow_to_color(gt)[1])
    M, N, _ = flo.shape
    rng = np.random.default_rng(0)
    up = lambda x: torch.from_numpy(np.asfortranarray(x)).to(dev)
    flow, var = up(flo), up(rng.uniform(0.25, 4.0, flo.shape))
    mu0 = up(flo + rng.normal(0, 0.1, flo.shape))
    mu, sg, rou = _fortran_dev((M, N, 2), dev), _fortran_dev((M, N, 2), dev), _fortran_dev((M, N, 2, 2), dev)
    o = cpu_options(dict(its=ITS, K=9))
    done = C.c_int(0)
    p = lambda t: C.c_void_p(t.data_ptr())
    vp = C.c_void_p

    def cpu_run(l):
        f = l.gqmap_cpu_run_device
        f.restype, f.argtypes = C.c_int, [C.c_void_p, vp, C.c_int, C.c_int, vp, C.c_uint64, vp, vp, vp, vp,
                                          C.POINTER(C.c_int), C.c_int]
        return lambda: f(C.byref(o), p(flow), M, N, None, 0, p(mu), p(sg), p(rou), None, C.byref(done), 0)

    def denoise(v, m0, scatter):
        f = lib.gqmap_flow_denoise_device
        return lambda: f(C.byref(o), flow.data_ptr(), v, m0, M, N, None, 0, scatter, mu.data_ptr(), sg.data_ptr(),
                         rou.data_ptr(), None, C.byref(done), 0)

    variants = []
    if a.parent_lib:
        variants.append(("parent", cpu_run(C.CDLL(os.path.abspath(a.parent_lib)))))
    variants += [("cpu_run", cpu_run(lib)), ("ref", denoise(None, None, _lib.SCATTER_REFERENCE)),
                 ("field", denoise(var.data_ptr(), mu0.data_ptr(), _lib.SCATTER_ADJOINT))]
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < WARM_S:
        for name, call in variants:
            if call() != 0 or done.value != ITS:
                raise SystemExit(f"{name}: status / its_done {done.value}: {lib.gqmap_last_error()}")
    ms = {name: [] for name, _ in variants}
    for _ in range(ROUNDS):
        for name, call in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = call()
            e1.record()
            e1.synchronize()
            if rc != 0:
                raise SystemExit(f"{name}: status {rc}")
            ms[name].append(e0.elapsed_time(e1))
    lines = [f"flow denoising, {M} x {N}, K = 9, {ITS} iterations, device arrays; HIP events, {WARM_S} s warm-up, "
             f"median of {ROUNDS} interleaved calls (min .. max), ms per call",
             f"device: {torch.cuda.get_device_name(0)}"]
    for name, _ in variants:
        v = sorted(ms[name])
        lines.append(f"{name:8s} {v[len(v) // 2]:8.3f}  ({v[0]:.3f} .. {v[-1]:.3f})")
    if not a.parent_lib:
        lines.append("parent   not measured (no --parent-lib)")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
