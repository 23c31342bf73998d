"""Python mirror of the reference engines' call signature, over the C ABI.

    mu, sigma, alpha, AEPE, Energy, logP = gqmap_gpu_mixture(options, I1, I2)
        -- gqmap_gpu_mixture.m:1 (optical_flow.m:27)
    mu, sigma, alpha, AEPE, Energy, logP = gqmap_gpuSuper_mix_entropy(options, I1, I2)
        -- gqmap_gpuSuper_mix_entropy.m:1 (optical_flowSuper.m:34)

`options` is a dict with the MATLAB field names (trueFlow, unknownIdx, its,
K, L, temperature, drate, epsn, lambdad, lambdas, minu, maxu, minv, maxv,
dir).  The solver loop runs on the GPU (libgqmap.so); the host keeps what the
reference keeps on the host: the evaluation block every 300 iterations
(gqmap_gpu_mixture.m:52-68: MAP, flowToColor, PNG, AEPE, logP) and the
per-iteration console line.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import check, dptr, f64
from .ops import flow_to_color

ENGINES = {"mixture": _lib.ENGINE_MIXTURE, "super": _lib.ENGINE_SUPER, "ctf": _lib.ENGINE_CTF}
PRECISIONS = {"fp64": _lib.FP64, "fp32": _lib.FP32}
KNOBS = ("alpha_mode", "alpha_start", "alpha_lr", "guard_a", "t_decay_every", "t_min", "step0",
         "step_decay", "sig_lo", "sig_hi", "corr_tor", "tor", "split", "sig_step", "sig_init", "arith")
ARITH = {"fast": _lib.ARITH_FAST, "literal": _lib.ARITH_LITERAL}


def make_options(options: dict, engine: str = "mixture", precision: str = "fp64") -> _lib.GqmapOptions:
    lib = _lib.load()
    o = _lib.GqmapOptions()
    lib.gqmap_options_default(C.byref(o), ENGINES[engine])
    for k in ("its", "K", "L"):
        if k in options:
            setattr(o, k, int(options[k]))
    for k in ("temperature", "drate", "epsn", "lambdad", "lambdas", "minu", "maxu", "minv", "maxv"):
        if k in options:
            setattr(o, k, float(options[k]))
    o.engine = ENGINES[engine]
    if "alpha_mode" in options:  # the mode's reference alpha_start / alpha_lr, unless given below
        check(lib.gqmap_options_alpha_mode(C.byref(o), int(options["alpha_mode"])), "alpha_mode")
    for k in KNOBS:
        if k in options:
            cur = getattr(o, k)
            v = options[k]
            if k == "arith" and isinstance(v, str):
                v = ARITH[v]
            setattr(o, k, type(cur)(v))
    o.engine = ENGINES[engine]
    o.precision = PRECISIONS[precision]
    return o


@dataclass
class State:
    """Engine state in MATLAB layout (M x N x L, rou M x N x L x 2 x 2)."""
    muu: np.ndarray
    muv: np.ndarray
    sigu: np.ndarray
    sigv: np.ndarray
    pn: np.ndarray
    rou: np.ndarray
    w: np.ndarray
    alpha: np.ndarray
    it: int = 1
    T: float = 0.0

    def cstruct(self) -> _lib.GqmapState:
        s = _lib.GqmapState()
        for k in ("muu", "muv", "sigu", "sigv", "pn", "rou", "w", "alpha"):
            setattr(s, k, dptr(getattr(self, k)))
        s.it, s.T = int(self.it), float(self.T)
        return s

    @staticmethod
    def empty(M: int, N: int, L: int) -> "State":
        z = lambda *sh: np.zeros(sh, order="F")
        return State(z(M, N, L), z(M, N, L), z(M, N, L), z(M, N, L), z(M, N, L),
                     z(M, N, L, 2, 2), np.zeros(L), np.zeros(L))

    def copy(self) -> "State":
        return State(*(np.array(getattr(self, k), order="F", copy=True) for k in
                       ("muu", "muv", "sigu", "sigv", "pn", "rou", "w", "alpha")), self.it, self.T)


def rand_uniform(seed: int, stream: int, n: int, first: int = 0) -> np.ndarray:
    """The library's counter-based U(0,1) stream (host evaluation)."""
    out = np.empty(n)
    _lib.load().gqmap_rand_uniform(C.c_uint64(seed), C.c_uint32(stream), C.c_uint64(first),
                                   C.c_size_t(n), dptr(out))
    return out


def initial_state(options: dict, M: int, N: int, seed: int = 0, T: float | None = None,
                  engine: str = "mixture", flow=None, sigma=None) -> State:
    """Host copy of gqmap_init_state: gqmap_gpu_mixture.m:18-24 with the
    library RNG (what the device generates for the same seed).  With a flow
    (M x N x 2 on the node grid) the host copy of gqmap_init_state_flow:
    component 0 of the mean is the flow clamped to the range; NaN and
    |x| > 1e9 entries keep the draw.  With M x N x 2 x H the host copy of
    gqmap_init_state_flows: component l < H takes slice l in the same way.
    With sigma as well (shaped as flow, plane 0 = sigma_u, plane 1 = sigma_v)
    the host copy of gqmap_init_state_seeded: a finite entry > 0 puts
    min(max(x, sig_lo), sig_hi) into component l < H of sigu / sigv; NaN, <= 0
    and Inf entries keep the draw."""
    L = int(options["L"])
    MNL = M * N * L
    sh = lambda a: a.reshape((M, N, L), order="F")
    w = rand_uniform(seed, 0, L)
    du, dv = options["maxu"] - options["minu"], options["maxv"] - options["minv"]
    # sigma offset: (max-min) for the mixture engines, 3 for ctf (gqmap_ctf.m:16-17)
    sig_init = float(options.get("sig_init", 3.0 if engine == "ctf" else -1.0))
    su, sv = (du, dv) if sig_init < 0 else (sig_init, sig_init)
    st = State(
        muu=sh(options["minu"] + rand_uniform(seed, 1, MNL) * du),
        muv=sh(options["minv"] + rand_uniform(seed, 2, MNL) * dv),
        sigu=sh(rand_uniform(seed, 3, MNL) + su),
        sigv=sh(rand_uniform(seed, 4, MNL) + sv),
        pn=np.zeros((M, N, L), order="F"), rou=np.zeros((M, N, L, 2, 2), order="F"),
        w=w, alpha=np.exp(w) / np.exp(w).sum(), it=1,
        T=float(options.get("temperature", 0.0) if T is None else T))
    if flow is not None:
        flow = np.asarray(flow, dtype=np.float64)
        if flow.ndim == 3:
            flow = flow[:, :, :, None]
        if flow.shape[:3] != (M, N, 2) or flow.ndim != 4 or not 1 <= flow.shape[3] <= L:
            raise ValueError(f"flow must be {M}x{N}x2 or {M}x{N}x2xH with H <= L, got {flow.shape}")
        for l in range(flow.shape[3]):
            for plane, x, lo, hi in ((st.muu, flow[:, :, 0, l], options["minu"], options["maxu"]),
                                     (st.muv, flow[:, :, 1, l], options["minv"], options["maxv"])):
                with np.errstate(invalid="ignore"):
                    known = ~(np.isnan(x) | (np.abs(x) > 1e9))
                    plane[:, :, l] = np.where(known, np.minimum(np.maximum(x, lo), hi), plane[:, :, l])
    if sigma is not None:
        if flow is None:
            raise ValueError("sigma needs a flow")
        sigma = np.asarray(sigma, dtype=np.float64)
        if sigma.ndim == 3:
            sigma = sigma[:, :, :, None]
        if sigma.shape != flow.shape:
            raise ValueError(f"sigma shape {sigma.shape} != flow shape {flow.shape}")
        o = make_options(options, engine)
        for l in range(sigma.shape[3]):
            for plane, x in ((st.sigu, sigma[:, :, 0, l]), (st.sigv, sigma[:, :, 1, l])):
                with np.errstate(invalid="ignore"):
                    given = np.isfinite(x) & (x > 0)
                    plane[:, :, l] = np.where(given, np.minimum(np.maximum(x, o.sig_lo), o.sig_hi), plane[:, :, l])
    return st


class Engine:
    """One device context (gqmap_ctx) holding images and state on the GPU."""

    def __init__(self, options: dict, I1, I2, engine: str = "mixture", precision: str = "fp64",
                 device: int = 0, n_tiles: int = 1, tile: int = 0):
        self.lib = _lib.load()
        self.engine, self.precision = engine, precision
        self.opts = make_options(options, engine, precision)
        self.ctx = C.c_void_p()
        if n_tiles == 1:
            check(self.lib.gqmap_create(C.byref(self.ctx), C.byref(self.opts), device), "gqmap_create")
        else:
            check(self.lib.gqmap_create_tile(C.byref(self.ctx), C.byref(self.opts), device, n_tiles, tile),
                  "gqmap_create_tile")
        I1, I2 = f64(I1), f64(I2)
        if I1.shape != I2.shape or I1.ndim != 2:
            raise ValueError("I1 and I2 must be equal-size 2-D images")
        self.Mo, self.No = I1.shape
        check(self.lib.gqmap_set_images(self.ctx, dptr(I1), dptr(I2), self.Mo, self.No),
              "gqmap_set_images")
        info = self.info()
        self.M, self.N, self.L = info.M, info.N, info.L  # full node grid (a tile owns col0:col1)
        self.n_tiles, self.tile, self.col0, self.col1 = info.n_tiles, info.tile, info.col0, info.col1

    # -- multi-GPU tiles ---------------------------------------------------
    def attach_rccl(self, unique_id: bytes) -> None:
        """Join the RCCL communicator of all tiles (rank == tile); collective."""
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        check(self.lib.gqmap_tile_attach_rccl(self.ctx, buf), "gqmap_tile_attach_rccl")

    def attach_host(self) -> None:
        """Host-staged transport (gqmap_tile_attach_host): the caller moves
        the boundary columns and totals between exchange_begin / _end."""
        check(self.lib.gqmap_tile_attach_host(self.ctx), "gqmap_tile_attach_host")
        sz = (C.c_size_t * 6)()
        check(self.lib.gqmap_tile_exchange_sizes(self.ctx, sz), "gqmap_tile_exchange_sizes")
        # send_left, send_right, recv_left, recv_right, totals, totals_all (bytes)
        self.xfer_sizes = tuple(int(v) for v in sz)

    def exchange_begin(self):
        """One iteration up to the exchange: (send_left, send_right, totals)
        as uint8 arrays (send_* empty at the strip ends)."""
        sl, sr, _, _, tot, _ = self.xfer_sizes
        bufs = [np.zeros(n, np.uint8) for n in (sl, sr, tot)]
        ptrs = [b.ctypes.data_as(C.c_void_p) if b.size else None for b in bufs]
        check(self.lib.gqmap_tile_exchange_begin(self.ctx, *ptrs), "gqmap_tile_exchange_begin")
        return tuple(bufs)

    def exchange_end(self, recv_left, recv_right, totals_all) -> np.ndarray:
        """Finish the iteration with the neighbours' columns (recv_left from
        tile-1's send_right, recv_right from tile+1's send_left) and every
        tile's totals in tile order.  Returns Energy, ptdmu, ptdsigma."""
        tr = np.zeros(3)
        bufs = [np.ascontiguousarray(b, np.uint8) if b is not None else None
                for b in (recv_left, recv_right, totals_all)]
        for b, n, what in zip(bufs, self.xfer_sizes[2:4] + self.xfer_sizes[5:], ("recv_left", "recv_right", "totals_all")):
            if n and (b is None or b.size != n):
                raise ValueError(f"{what} must hold {n} bytes")
        ptrs = [b.ctypes.data_as(C.c_void_p) if b is not None and b.size else None for b in bufs]
        check(self.lib.gqmap_tile_exchange_end(self.ctx, *ptrs, dptr(tr)), "gqmap_tile_exchange_end")
        return tr

    # -- state -----------------------------------------------------------
    def init_state(self, seed: int = 0) -> None:
        check(self.lib.gqmap_init_state(self.ctx, C.c_uint64(seed)), "gqmap_init_state")

    def init_state_from_flow(self, flow, seed: int = 0, sigma=None) -> None:
        """gqmap_init_state_flow: init_state(seed) with component 0 of the mean
        set to `flow` (full node grid M x N x 2) clamped to the options' range.
        A flow M x N x 2 x H (H <= L, e.g. from block_match_init(hypotheses=H))
        seeds components 0..H-1 from its slices (gqmap_init_state_flows).
        sigma (shaped as flow, e.g. from block_match_init(sigma_from_cost=True))
        also sets sigu / sigv of those components, clamped to [sig_lo, sig_hi],
        where it is finite and > 0 (gqmap_init_state_seeded)."""
        flow = f64(flow)
        if sigma is not None:
            sigma = f64(sigma)
            if sigma.shape != flow.shape or flow.ndim not in (3, 4) or flow.shape[:3] != (self.M, self.N, 2):
                raise ValueError(f"flow {flow.shape} and sigma {sigma.shape} must both be the node grid "
                                 f"{(self.M, self.N, 2)} (x H)")
            H = int(flow.shape[3]) if flow.ndim == 4 else 1
            check(self.lib.gqmap_init_state_seeded(self.ctx, dptr(flow), dptr(sigma), H, C.c_uint64(seed)),
                  "gqmap_init_state_seeded")
            return
        if flow.ndim == 4 and flow.shape[:3] == (self.M, self.N, 2):
            check(self.lib.gqmap_init_state_flows(self.ctx, dptr(flow), int(flow.shape[3]), C.c_uint64(seed)),
                  "gqmap_init_state_flows")
            return
        if flow.shape != (self.M, self.N, 2):
            raise ValueError(f"flow shape {flow.shape} != node grid {(self.M, self.N, 2)} (x H)")
        check(self.lib.gqmap_init_state_flow(self.ctx, dptr(flow), C.c_uint64(seed)), "gqmap_init_state_flow")

    def set_state(self, st: State) -> None:
        for k in ("muu", "muv", "sigu", "sigv", "pn", "rou", "w", "alpha"):
            setattr(st, k, f64(getattr(st, k)))
        exp = (self.M, self.N, self.L)
        if st.muu.shape != exp or st.rou.shape != exp + (2, 2):
            raise ValueError(f"state shape {st.muu.shape} != node grid {exp}")
        cs = st.cstruct()
        check(self.lib.gqmap_set_state(self.ctx, C.byref(cs)), "gqmap_set_state")

    def get_state(self) -> State:
        st = State.empty(self.M, self.N, self.L)
        cs = st.cstruct()
        check(self.lib.gqmap_get_state(self.ctx, C.byref(cs)), "gqmap_get_state")
        st.it, st.T = cs.it, cs.T
        return st

    # -- iterations ------------------------------------------------------
    def run(self, n_iter: int):
        """Run up to n_iter iterations; returns (n_done, trace[n_done, 3])."""
        trace = np.zeros((max(n_iter, 1), 3))
        done = C.c_int(0)
        check(self.lib.gqmap_run(self.ctx, int(n_iter), C.byref(done), dptr(trace)), "gqmap_run")
        return done.value, trace[:done.value]

    def set_truth(self, grdt) -> None:
        """Ground truth of the ctf level engine (gqmap_set_truth): GRDT of
        gqmap_ctf(options,I1,I2,GRDT), Mg x Ng x 2 with Mg >= M, Ng >= N (its
        top-left M x N block is used, as gqmap_ctf.m:38 does); None clears."""
        if grdt is None:
            check(self.lib.gqmap_set_truth(self.ctx, None, 0, 0), "gqmap_set_truth")
            return
        g = f64(grdt)
        if g.ndim != 3 or g.shape[2] != 2:
            raise ValueError("truth must be Mg x Ng x 2")
        check(self.lib.gqmap_set_truth(self.ctx, dptr(g), g.shape[0], g.shape[1]), "gqmap_set_truth")

    def run_aepe(self, n_iter: int):
        """run() plus the per-iteration AEPE of gqmap_ctf.m:38 (NaN without a
        truth): (n_done, trace[n_done, 3], aepe[n_done])."""
        trace = np.zeros((max(n_iter, 1), 3))
        ae = np.zeros(max(n_iter, 1))
        done = C.c_int(0)
        check(self.lib.gqmap_run_aepe(self.ctx, int(n_iter), C.byref(done), dptr(trace), dptr(ae)),
              "gqmap_run_aepe")
        return done.value, trace[:done.value], ae[:done.value]

    def run_timed(self, n_iter: int):
        done, tot, ker = C.c_int(0), C.c_double(0), C.c_double(0)
        check(self.lib.gqmap_run_timed(self.ctx, int(n_iter), C.byref(done), C.byref(tot),
                                       C.byref(ker)), "gqmap_run_timed")
        return done.value, tot.value, ker.value

    def prepare(self) -> None:
        """Build and upload the replayed iteration graph now (gqmap_prepare)."""
        check(self.lib.gqmap_prepare(self.ctx), "gqmap_prepare")

    def dataflow(self) -> bool:
        """Whether runs take the dataflow launch (k_iter_flow, one launch per
        chunk of FLOW_CHUNK iterations) rather than one k_iter launch per iteration
        (gqmap_debug_flow; the library's flow policy)."""
        f = self.lib.gqmap_debug_flow
        f.restype = C.c_int
        f.argtypes = [C.c_void_p]
        return bool(f(self.ctx))

    def persistent(self) -> bool:
        """Whether runs take the persistent launch (k_iter_persist, a chunk of
        iterations per launch behind a grid barrier: the small ctf levels;
        gqmap_debug_persist).  It is tried before the dataflow launch."""
        f = self.lib.gqmap_debug_persist
        f.restype = C.c_int
        f.argtypes = [C.c_void_p]
        return bool(f(self.ctx))

    def synchronize(self) -> None:
        check(self.lib.gqmap_synchronize(self.ctx), "gqmap_synchronize")

    def info(self) -> _lib.GqmapInfo:
        inf = _lib.GqmapInfo()
        check(self.lib.gqmap_get_info(self.ctx, C.byref(inf)), "gqmap_get_info")
        return inf

    def map(self) -> np.ndarray:
        out = np.zeros((self.M, self.N, 2), order="F")
        check(self.lib.gqmap_get_map(self.ctx, dptr(out)), "gqmap_get_map")
        return out

    def log_p(self, map_: np.ndarray) -> float:
        v = C.c_double(0)
        check(self.lib.gqmap_log_p(self.ctx, dptr(f64(map_)), C.byref(v)), "gqmap_log_p")
        return v.value

    def close(self) -> None:
        if self.ctx:
            self.lib.gqmap_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def strip_split(M: int, N: int, n_tiles: int) -> int:
    """Lanes per node Q for a single-scale mixture grid M x N cut into n_tiles
    column strips, chosen from ONE strip's node count with the library's own
    thresholds (gqmap_engine.hip choose_split, mixture: Q = 1 from 98,304
    nodes, 2 from 2^14, 4 from 2^13, 8 from 2^11, else 64 -- one wave per
    node).  The library picks Q from the whole grid so a tiled solve sums in
    the untiled order; pass this as options["split"] to every tile AND to the
    whole-grid reference to keep both bit-identical while each rank's strip
    still fills the GPU (strong scaling).  tests/test_tiles.py pins these
    thresholds against the library's."""
    nodes = M * -(-N // max(1, n_tiles))
    return (1 if nodes >= 98304 else 2 if nodes >= 1 << 14 else 4 if nodes >= 1 << 13
            else 8 if nodes >= 1 << 11 else 64)


def comm_unique_id() -> bytes:
    """An RCCL unique id for Engine.attach_rccl (draw on one rank, broadcast)."""
    buf = (C.c_uint8 * 128)()
    check(_lib.load().gqmap_comm_unique_id(buf), "gqmap_comm_unique_id")
    return bytes(buf)


def tile_group_run(tiles, n_iter: int):
    """Run the tiles of one grid (same device, tile order) n_iter iterations in
    lockstep with in-process halo exchange.  Returns (n_done, trace)."""
    lib = _lib.load()
    arr = (C.c_void_p * len(tiles))(*[t.ctx.value for t in tiles])
    trace = np.zeros((max(n_iter, 1), 3))
    done = C.c_int(0)
    check(lib.gqmap_tile_group_run(arr, len(tiles), int(n_iter), C.byref(done), dptr(trace)),
          "gqmap_tile_group_run")
    return done.value, trace[:done.value]


def aepe(tflow: np.ndarray, flow: np.ndarray, unknown: np.ndarray, crop: int = 1) -> float:
    """gqmap_gpu_mixture.m:63-64: flow(unidx)=0; mean over the interior of
    the end-point error (super engine: crop=4, gqmap_gpuSuper_mix_entropy.m:63)."""
    f = np.array(flow, dtype=np.float64)
    f[np.asarray(unknown, dtype=bool)] = 0
    M, N = f.shape[:2]
    sl = (slice(crop, M - crop), slice(crop, N - crop))
    d = tflow[sl] - f[sl]
    return float(np.mean(np.mean(np.sqrt(np.sum(d ** 2, axis=2)), axis=0)))


def _solve(engine: str, options: dict, I1, I2, *, seed: int = 0, precision: str = "fp64",
           device: int = 0, state: State | None = None, verbose: bool = False,
           eval_every: int = 300, init_flow=None, init_sigma=None):
    its = int(options["its"])
    L = int(options["L"])
    sup = engine == "super"
    tflow = options.get("trueFlow")
    unk = options.get("unknownIdx")
    odir = options.get("dir")
    AEPE = np.full(its, np.nan)
    logP = np.full(its, np.nan)
    Energy = np.zeros(its)
    best = np.inf
    mark = None
    if init_sigma is not None and init_flow is None:
        raise ValueError("init_sigma needs init_flow")
    with Engine(options, I1, I2, engine, precision, device) as eng:
        if state is not None:
            eng.set_state(state)
        elif init_flow is not None:
            eng.init_state_from_flow(init_flow, seed, init_sigma)
        else:
            eng.init_state(seed)
        it = 1
        while it <= its:
            # run up to the next evaluation point (it == 1 or it % eval_every == 0)
            nxt = 1 if it == 1 else min(its, (it // eval_every + 1) * eval_every)
            n = nxt - it + 1
            done, tr = eng.run(n)
            Energy[it - 1: it - 1 + done] = tr[:, 0]
            last = it + done - 1
            if done == n and (last == 1 or last % eval_every == 0):
                mp = eng.map()
                flow = np.repeat(np.repeat(mp, 4, axis=0), 4, axis=1) if sup else mp
                crop = 4 if sup else 1
                img = flow_to_color(flow[4:-4, 4:-4] if sup else flow, device=device)[0]
                if odir:
                    from .flowio import imwrite
                    os.makedirs(odir, exist_ok=True)
                    imwrite(img, os.path.join(odir, f"{last}.png"))
                if tflow is not None:
                    a = aepe(tflow, flow, unk, crop)
                    AEPE[last - 1] = a
                    best = min(best, a)
                logP[last - 1] = eng.log_p(mp)
                mark = last
            if verbose:
                for k in range(done):
                    print(f"[{it + k:3d}], Δ(mu) = {tr[k, 1]:e}, Δ(sigma) = {tr[k, 2]:e}, "
                          f"Energy = {tr[k, 0]:e}, AEPE={best:e},logP={logP[mark - 1] if mark else np.nan:e}")
            it += done
            if done < n:  # ptdmu < tor
                break
        st = eng.get_state()
    mu = np.stack([st.muu, st.muv], axis=3)
    sigma = np.stack([st.sigu, st.sigv], axis=3)
    alpha = st.alpha.reshape(1, 1, L)
    return mu, sigma, alpha, AEPE, Energy, logP


def gqmap_gpu_mixture(options: dict, I1, I2, **kw):
    """[mu, sigma, alpha, AEPE, Energy, logP] = gqmap_gpu_mixture(options, I1, I2)."""
    return _solve("mixture", options, I1, I2, **kw)


def gqmap_gpuSuper_mix_entropy(options: dict, I1, I2, **kw):
    """[mu, sigma, alpha, AEPE, Energy, logP] = gqmap_gpuSuper_mix_entropy(options, I1, I2)."""
    return _solve("super", options, I1, I2, **kw)


def block_match_init(I1, I2, U: int = 7, V: int = 7, ft: int = 3, sigma: float = 1.7,
                     engine: str = "mixture", device: int = 0, host: bool = False,
                     hypotheses: int | None = None, sep: int = 2, subpixel: bool = False,
                     sigma_from_cost: bool = False, lambdad: float = 1.0, sigma_min: float = 0.5,
                     consistency: bool = False, fill: bool = False, fb_a1: float = 0.01, fb_a2: float = 0.5,
                     fill_r: int = 8, fill_sigma: float = 4.0, fill_passes: int = 2, levels: int = 1, pyr_r: int = 1,
                     pyr_k: int = 1, pyr_ranked: bool = False):
    """A start and a range for the engines from two frames alone
    (legacy/optical_flow_temp.m:13-32; defaults: the reference's at scale 1,
    U = floor(6*scale)+1).  The engine's data term compares I1(i, j) with I2 at
    (i + v, j + u) -- a flow on I1's grid -- so this is block_match(A=I1, B=I2)
    negated.  Returns (flow, ranges): flow on the node grid (engine="super":
    the mean of each 4 x 4 block), ranges = dict(minu, maxu, minv, maxv) to merge
    into the options; pass flow as init_flow= / Engine.init_state_from_flow.

    hypotheses=H returns M x N x 2 x H, one flow per mixture component (ranks of
    block_match(hypotheses=H, sep=sep), negated; a missing rank stays NaN and
    keeps the random draw).  engine="super": rank 0 is the block mean as above,
    whatever H.  A node's rank k >= 1 is the rank-k flow of the ONE pixel of its
    4 x 4 block whose rank-k cost is smallest (ties: the first pixel in
    column-major order of the block; NaN when no pixel of the block has that
    rank).  It is not a mean: the rank-k picks of different pixels are
    unrelated modes, and averaging them would blend them into a displacement
    that none of the pixels proposed.

    subpixel=True takes the flows of block_match(subpixel=True) instead (each
    axis moved by up to half a pixel along the parabola through the pick's cost
    and its two neighbours'), negated as above; shapes as without it.  The
    ranges stay +-V / +-U.  sigma_from_cost=True (needs subpixel) returns
    (flow, ranges, sigma), sigma shaped as flow, plane 0 = sigma_u, for init_sigma=
    / Engine.init_state_from_flow(sigma=): under the engine's data term
    -lambdad |dI| per pixel the parabola's curvature curv is a Laplace estimate
    of the precision of the mean proposed, so sigma = max(sqrt(1 / (lambdad
    curv)), sigma_min) where curv > 0 and NaN (keeps the draw) elsewhere.
    sigma_min = 0.5 because a three-point fit on an integer grid cannot certify
    less than half a pixel; it is a knob, not a measured optimum.
    engine="super": rank 0's curvature is the SUM over the 4 x 4 block (the
    node's data term sums its 16 pixels, and precisions add) beside the block
    mean of the refined flows; rank k >= 1 takes flow and curvature of the one
    cheapest pixel, by the rule above.

    consistency=True adds a forward-backward check, all of it on the pixel grid
    (engine="super": before the nodes are formed).  The matcher also runs
    backward, block_match_init(I2, I1) with the same U, V, ft, sigma and subpixel
    and one hypothesis, and every forward rank k is checked against that flow by
    flow_consistency(a1=fb_a1, a2=fb_a2); a missing rank is inconsistent.  Where
    rank k is inconsistent its flow becomes NaN (keeps the random draw), the cost
    of a rank k >= 1 becomes +Inf and its curvature 0, so sigma is NaN there.
    fill=True (needs consistency) gives rank 0 at an inconsistent pixel the value
    of flow_fill(r=fill_r, sigma=fill_sigma, passes=fill_passes) over the
    consistent rank-0 pixels instead; a pixel still unfilled stays NaN.  A filled
    flow is a guess that no curvature certified: its sigma stays NaN, the wide
    draw.  engine="super": rank 0 of a node is the mean over the non-NaN pixels
    of its block (NaN when there are none) and its curvature the sum over the
    consistent pixels; ranks k >= 1 keep the cheapest-pixel rule, which the +Inf
    costs now steer.  The boolean `consistent` (pixel grid: M x N x H, M x N
    without hypotheses) is appended as the last element of the return.  With
    consistency=False every output is what it was without these keywords.

    levels > 1 takes rank 0 from the coarse-to-fine matcher instead,
    block_match_pyramid(levels=levels, r=pyr_r, k=pyr_k), forward and, with
    consistency=True, backward; subpixel, sigma_from_cost, consistency, fill and
    engine="super" work on it as on rank 0 above, shapes unchanged.  U and V may
    then exceed 32 (ceil(U / 2^(levels-1)) <= 32) and the ranges become
    +-block_match_reach(V, levels, pyr_r) / +-block_match_reach(U, levels, pyr_r).
    By default it yields one hypothesis per pixel: hypotheses > 1 raises
    ValueError.  With levels=1 every output is what it was without these
    keywords.

    pyr_ranked=True (with levels > 1 and hypotheses=H) takes rank k from the
    ranked coarse-to-fine matcher, block_match_pyramid(levels=levels, r=pyr_r,
    k=pyr_k, hypotheses=H, sep=sep): every rank is handed down the levels in a
    box of its own, rank 0 is the flow without pyr_ranked, and a rank missing at
    a pixel stays NaN.  Only the forward pass is ranked; the backward pass of
    consistency=True stays the plain pyramid with one hypothesis.  subpixel,
    sigma_from_cost, consistency, fill and engine="super" apply to the ranks as
    they do at levels=1, and the ranges stay +-block_match_reach."""
    from .ops import block_match, block_match_pyramid, block_match_reach, flow_consistency, flow_fill
    sup = engine == "super"
    if sigma_from_cost and not subpixel:
        raise ValueError("block_match_init: sigma_from_cost needs subpixel=True")
    if fill and not consistency:
        raise ValueError("block_match_init: fill needs consistency=True")
    if sup and (np.shape(I1)[0] % 4 or np.shape(I1)[1] % 4):
        raise ValueError("super engine: image size must be divisible by 4")
    if levels > 1 and hypotheses is not None and hypotheses > 1 and not pyr_ranked:
        raise ValueError("block_match_init: levels > 1 yields one hypothesis per pixel (pyr_ranked=True: one per rank)")
    if levels > 1:
        ru, rv = (float(block_match_reach(x, levels, pyr_r)) for x in (U, V))
        ranges = dict(minu=-rv, maxu=rv, minv=-ru, maxv=ru)

        def match(A, B, **kw):  # rank 0 with the rank axis block_match gives it
            if pyr_ranked and kw.get("hypotheses") is not None:  # the forward pass: the ranks come with their axis
                return block_match_pyramid(A, B, U, V, ft, sigma, levels, pyr_r, pyr_k, subpixel=subpixel,
                                           device=device, host=host, **kw)
            got = block_match_pyramid(A, B, U, V, ft, sigma, levels, pyr_r, pyr_k, subpixel=subpixel, device=device,
                                      host=host)
            ranked = hypotheses is not None or subpixel
            return tuple(np.asfortranarray(a[..., None]) for a in got) if ranked else got
    else:
        ranges = dict(minu=float(-V), maxu=float(V), minv=float(-U), maxv=float(U))

        def match(A, B, **kw):
            return block_match(A, B, U, V, ft, sigma, device=device, host=host, subpixel=subpixel, **kw)
    out, cost, *curv = match(I1, I2, hypotheses=hypotheses, sep=sep)
    flow, curv = np.asfortranarray(0.0 - out), curv[0] if subpixel else None
    if flow.ndim == 3:  # without hypotheses or subpixel block_match leaves the rank axis out
        flow, cost = flow[..., None], cost[..., None]
    tail = ()
    if consistency:
        back = match(I2, I1)[0]
        bwd = np.asfortranarray((0.0 - back).reshape(back.shape[:3], order="F"))
        # a NaN flow (a missing rank) has no target inside the frame: inconsistent
        cons = np.stack([flow_consistency(flow[:, :, :, k], bwd, fb_a1, fb_a2, device=device, host=host)[1]
                         for k in range(flow.shape[3])], axis=2)
        if fill:
            flow[:, :, :, 0], state = flow_fill(flow[:, :, :, 0], cons[:, :, 0], fill_r, fill_sigma, fill_passes,
                                                device=device, host=host)
            flow[:, :, :, 0][state == 255] = np.nan
        else:
            flow[:, :, :, 0][~cons[:, :, 0]] = np.nan
        for k in range(1, flow.shape[3]):
            flow[:, :, :, k][~cons[:, :, k]] = np.nan
            cost[:, :, k][~cons[:, :, k]] = np.inf
        if curv is not None:
            curv[np.broadcast_to(~cons[:, :, None, :], curv.shape)] = 0.0
        tail = (np.asfortranarray(cons[:, :, 0] if hypotheses is None else cons),)
    if sup:
        nodes = _super_hypotheses(flow, cost, curv, _mean_of_known if consistency else np.mean)
        flow, curv = nodes if subpixel else (nodes, None)
    if hypotheses is None:
        flow = np.asfortranarray(flow[:, :, :, 0])
    if not sigma_from_cost:
        return (flow, ranges) + tail
    if hypotheses is None:
        curv = curv[:, :, :, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        sig = np.where(curv > 0, np.maximum(np.sqrt(1.0 / (float(lambdad) * curv)), float(sigma_min)), np.nan)
    return (flow, ranges, np.asfortranarray(sig)) + tail


def block_match_flow(I1, I2, U: int = 7, V: int = 7, ft: int = 3, sigma: float = 1.7, levels: int = 1, pyr_r: int = 1,
                     pyr_k: int = 1, var_scale: float = 1.0, var_default: float = 1.0, weighted: bool = True,
                     denoise: dict | None = None, device: int = 0, host: bool = False, median: dict | None = None):
    """A flow from two frames alone: the block-matching start, checked both
    ways and refilled, then denoised.  block_match_init(subpixel=True,
    sigma_from_cost=True, consistency=True, fill=True) with U, V, ft, sigma,
    levels, pyr_r and pyr_k passed through, then ops.flow_denoise on
      observation  the refilled rank-0 flow; weighted=True: NaN (unobserved)
                   where the pixel is inconsistent, so a refilled pixel is moved
                   by its neighbours alone;
      variance     var_scale * sigma^2 where the cost-derived sigma is finite,
                   var_default elsewhere; weighted=False: var_default everywhere;
      start        the refilled flow, 0.0 where it is still NaN.
    denoise: the options of flow_denoise (default its=40; the other knobs of
    gqmap_cpu), and optionally its keywords scatter, seed, sigma0 and
    check_step.  var_scale is a knob nobody has tuned: the cost-derived widths
    are Laplace estimates under the engine's data term, not calibrated errors.
    Returns (flow, sigma, consistent): the denoised mean and its width
    (M x N x 2) and the forward-backward verdict (M x N bool).  host=True runs
    every stage on the library's host models (no device; bit-identical).
    median: a dict of ops.flow_wmedian's keywords (r, sigma_s, sigma_c, passes,
    conf); the denoised mean then goes through flow_wmedian with I1 as guide
    before it is returned.  conf="sigma" stands for flow_confidence of the
    returned width.  median=None (the default) filters nothing."""
    from .ops import flow_denoise, flow_wmedian
    start, _, sig, cons = block_match_init(I1, I2, U, V, ft, sigma, device=device, host=host, subpixel=True,
                                           sigma_from_cost=True, consistency=True, fill=True, levels=levels,
                                           pyr_r=pyr_r, pyr_k=pyr_k)
    kw = dict(denoise or {})
    call = {k: kw.pop(k) for k in ("scatter", "seed", "sigma0", "check_step") if k in kw}
    kw.setdefault("its", 40)
    obs = np.where(cons[:, :, None], start, np.nan) if weighted else start
    with np.errstate(invalid="ignore"):
        var = np.where(np.isfinite(sig), float(var_scale) * sig * sig, float(var_default))
    if not weighted:
        var = np.full(start.shape, float(var_default))
    mu0 = np.where(np.isnan(start), 0.0, start)
    mu, sg, _ = flow_denoise(obs, var, mu0, options=kw, device=device, host=host, **call)
    if median is not None:
        mkw = dict(median)
        if isinstance(mkw.get("conf"), str):
            if mkw["conf"] != "sigma":
                raise ValueError(f"block_match_flow: median conf must be an array or 'sigma', got {mkw['conf']!r}")
            mkw["conf"] = flow_confidence(sg)
        mu = flow_wmedian(mu, I1, device=device, host=host, **mkw)
    return mu, sg, cons


def flow_confidence(sigma, s0: float = 1.0):
    """A confidence map for ops.flow_wmedian from a width per pixel and axis:
    1 / (1 + (su^2 + sv^2) / s0^2) of an M x N x 2 sigma, as block_match_flow,
    block_match_init(sigma_from_cost=True) and the engines return it.  A host
    numpy array in (0, 1]; NaN in gives NaN out, which flow_wmedian takes as
    weight 0.  s0, the width at which (with su = sv = s0 / sqrt(2)) the
    confidence is one half, is a knob nobody has tuned."""
    sigma = np.asarray(sigma, dtype=np.float64)
    if sigma.ndim != 3 or sigma.shape[2] != 2:
        raise ValueError("flow_confidence: sigma must be M x N x 2")
    if not (s0 > 0 and np.isfinite(s0)):
        raise ValueError("flow_confidence: s0 must be finite and > 0")
    su, sv = sigma[:, :, 0], sigma[:, :, 1]
    return np.asfortranarray(1.0 / (1.0 + (su * su + sv * sv) / (float(s0) * float(s0))))


def _mean_of_known(x, axis):
    """Mean over the entries that are not NaN; NaN where there are none."""
    known = ~np.isnan(x)
    count = known.sum(axis=axis)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(count > 0, np.where(known, x, 0.0).sum(axis=axis) / count, np.nan)


def _super_hypotheses(flow, cost, curv=None, mean=np.mean):
    """Pixel hypotheses (M x N x 2 x H, M x N x H) on the super node grid; the
    rule is in block_match_init's docstring.  With curv (shaped as flow) returns
    (flow, curv) on the node grid: the block sum at rank 0, the cheapest pixel's
    curvature at rank k >= 1 (0 when the whole block misses the rank).  mean
    forms rank 0's flow from the block (block_match_init(consistency=True): the
    mean over the pixels that are not NaN)."""
    M, N, _, H = flow.shape
    m4, n4 = M // 4, N // 4
    # block pixels in column-major order of the block: index i + 4 j
    cb = cost.reshape(m4, 4, n4, 4, H).transpose(0, 2, 3, 1, 4).reshape(m4, n4, 16, H)
    first = np.argmin(cb, axis=2)  # +Inf (missing) never beats a finite cost; first on ties

    def nodes(x, rank0):
        out = np.empty((m4, n4, 2, H), order="F")
        out[:, :, :, 0] = rank0(x[:, :, :, 0].reshape(m4, 4, n4, 4, 2), axis=(1, 3))
        xb = x.reshape(m4, 4, n4, 4, 2, H).transpose(0, 2, 3, 1, 4, 5).reshape(m4, n4, 16, 2, H)
        # a block that misses rank k altogether takes its first pixel: NaN flow, curvature 0
        out[:, :, :, 1:] = np.take_along_axis(xb, first[:, :, None, None, :], axis=2)[:, :, 0, :, 1:]
        return out

    return nodes(flow, mean) if curv is None else (nodes(flow, mean), nodes(curv, np.sum))
