"""numpy restatement of csrc/gqmap_denoise.h (weighted flow denoising), written
from the header's specification: the same fp64 operations in the same order,
whole fields at a time.  Test infrastructure; shared inputs for
tests/test_flow_denoise.py and tests/test_gpu_flow_denoise.py."""
import numpy as np

PI = 3.14159265358979323846
SHAPES = [(37, 41), (5, 7), (2, 2), (3, 2), (61, 3)]


def abits_max(x):
    """The maximum of |x| taken on bit patterns (a NaN above +Inf), as a double."""
    return np.abs(np.ascontiguousarray(x)).view(np.uint64).max().view(np.float64)


def run(flow, var, mu0, sigma0, X, W, its, scatter="adjoint", var_scalar=1.0, gama=1.0, dta=np.inf, step0=0.1,
        step_decay=1000.0, corr=0.97, tor=1e-3, min_its=100):
    """Returns (mu, sigma, rou, trace[its_done, 3])."""
    flow = np.asarray(flow, dtype=np.float64)
    M, N, _ = flow.shape
    K = len(X)
    start = flow if mu0 is None else np.asarray(mu0, dtype=np.float64)
    if not np.isfinite(start).all():
        raise ValueError("the start must be finite")
    mu = np.array(start, order="F", copy=True)
    sigma = np.array(sigma0, dtype=np.float64, order="F", copy=True)
    rou = np.zeros((M, N, 2, 2), order="F")
    with np.errstate(invalid="ignore"):
        obs = np.isfinite(flow) if var is None else np.isfinite(flow) & np.isfinite(var) & (np.asarray(var) > 0)
    v = np.full(flow.shape, float(var_scalar)) if var is None else np.asarray(var, dtype=np.float64)
    sq2 = np.sqrt(2.0)
    WW = np.empty((K, K))
    for c in range(K):
        for r in range(K):
            WW[r, c] = W[c] * W[r]
    dnode = np.zeros((M, N, 2, 2))
    dedge = np.zeros((M, N, 2, 5, 2))
    trace = []
    I = (slice(0, M - 1), slice(0, N - 1))
    it = 1
    with np.errstate(all="ignore"):
        while True:
            o1, u1 = sigma[I], mu[I]
            so1 = sq2 * o1
            du, dsum = np.zeros_like(o1), np.zeros_like(o1)
            for k in range(K):
                x = so1 * X[k] + u1
                dval = np.where(obs[I], W[k] * (flow[I] - x) / v[I], 0.0)
                du = du + dval
                dsum = dsum + dval * X[k]
            dnode[I + (0,)] = du / np.sqrt(PI)
            dnode[I + (1,)] = dsum * np.sqrt(2.0 / PI)
            for j in range(2):
                J = (slice(1, M), slice(0, N - 1)) if j == 0 else (slice(0, M - 1), slice(1, N))
                o2, u2 = sigma[J], mu[J]
                p = rou[I + (j,)]
                so2 = sq2 * o2
                q, r = np.sqrt(1 + p), np.sqrt(1 - p)
                s, t = (q + r) / 2, (q - r) / 2
                ds, dt = (1 / q - 1 / r) / 4, (1 / q + 1 / r) / 4
                s1, so1s, so2s, sp = (np.zeros_like(p) for _ in range(4))
                for c in range(K):
                    sxi, txi, dsxi, dtxi = s * X[c], t * X[c], ds * X[c], dt * X[c]
                    c1, co1, co2, cp = (np.zeros_like(p) for _ in range(4))
                    for rr in range(K):
                        tx, sx, dtx, dsx = t * X[rr], s * X[rr], dt * X[rr], ds * X[rr]
                        ZI, ZJ = sxi + tx, txi + sx
                        x1, x2 = so1 * ZI + u1, so2 * ZJ + u2
                        diff = x2 - x1
                        diff = np.where(np.abs(diff) > dta, 0.0, diff)
                        df1 = WW[rr, c] * diff / gama
                        df2 = -df1
                        c1 = c1 + df1
                        co1 = co1 + df1 * ZI
                        co2 = co2 + df2 * ZJ
                        cp = cp + (o1 * df1 * (dsxi + dtx) + o2 * df2 * (dtxi + dsx))
                    s1, so1s, so2s, sp = s1 + c1, so1s + co1, so2s + co2, sp + cp
                dedge[I + (j, 0)] = 1 / PI * s1
                dedge[I + (j, 1)] = 1 / PI * (0.0 - s1)
                dedge[I + (j, 2)] = 1 / PI * sq2 * so1s
                dedge[I + (j, 3)] = 1 / PI * sq2 * so2s
                dedge[I + (j, 4)] = 1 / PI * sq2 * sp
            a = dnode[:, :, 0, :] + (dedge[:, :, 0, 0, :] + dedge[:, :, 1, 0, :])
            b = dnode[:, :, 1, :] + (dedge[:, :, 0, 2, :] + dedge[:, :, 1, 2, :])
            nu, nl, su, sl = (np.zeros((M, N, 2)) for _ in range(4))
            if scatter == "reference":
                nu[:M - 1], nl[:, :N - 1] = dedge[1:, :, 0, 1, :], dedge[:, 1:, 1, 1, :]
                su[:M - 1], sl[:, :N - 1] = dedge[1:, :, 0, 3, :], dedge[:, 1:, 1, 3, :]
            elif scatter == "adjoint":
                nu[1:], nl[:, 1:] = dedge[:M - 1, :, 0, 1, :], dedge[:, :N - 1, 1, 1, :]
                su[1:], sl[:, 1:] = dedge[:M - 1, :, 0, 3, :], dedge[:, :N - 1, 1, 3, :]
            else:
                raise ValueError(scatter)
            a = a + (nu + nl)
            b = b + (su + sl)
            step = step0 / (1 + it / step_decay)
            mu = mu + a * step
            sigma = np.abs(sigma + b * step)
            d = dedge[:, :, :, 4, :]
            rou = np.maximum(np.minimum(rou + d * step, corr), -corr)
            trace.append((abits_max(a), abits_max(b), abits_max(d)))
            if it + 1 > its or (it + 1 > min_its and trace[-1][0] < tor):
                break
            it += 1
    return np.asfortranarray(mu), np.asfortranarray(sigma), np.asfortranarray(rou), np.array(trace).reshape(-1, 3)


def run_options(flow, var, mu0, sigma0, X, W, options, scatter):
    """run() with the option names of gqmap_cpu_options."""
    o = dict(options)
    return run(flow, var, mu0, sigma0, X, W, o["its"], scatter=scatter, var_scalar=o.get("var", 1.0),
               gama=o.get("gama", 1.0), dta=o.get("dta", np.inf), step0=o.get("step0", 0.1),
               step_decay=o.get("step_decay", 1000.0), corr=o.get("corr_tor", 0.97), tor=o.get("tor", 1e-3),
               min_its=o.get("min_its", 100))


# ---- shared inputs --------------------------------------------------------------------

UNOBSERVED_KINDS = ("flow nan", "var +inf", "var nan", "var 0", "var -1")


def fields(shape, seed=0, layer_off=False):
    """(flow, var, mu0, sigma0) for a shape: var uniform in [0.25, 4]; about a fifth
    of the entries unobserved, every way of being so in turn (when the shape has
    at least five entries to spare); mu0 finite everywhere.  layer_off: the whole
    of layer 1 unobserved."""
    M, N = shape
    rng = np.random.default_rng(1000 * M + N + seed)
    clean = rng.normal(0, 2, (M, N, 2))
    flow = np.asfortranarray(clean + rng.normal(0, 0.5, (M, N, 2)))
    var = np.asfortranarray(rng.uniform(0.25, 4.0, (M, N, 2)))
    mu0 = np.asfortranarray(clean + rng.normal(0, 0.2, (M, N, 2)))
    sigma0 = np.asfortranarray(rng.uniform(0, 1, (M, N, 2)) + 2)
    off = rng.uniform(size=(M, N, 2)) < 0.2
    if layer_off:
        off[:, :, 1] = True
    idx = np.argwhere(off)
    if len(idx) < len(UNOBSERVED_KINDS):  # the smallest shapes: the first entries, one kind each
        idx = np.argwhere(np.ones((M, N, 2), dtype=bool))[:len(UNOBSERVED_KINDS)]
    for i, (m, n, l) in enumerate(idx):
        kind = UNOBSERVED_KINDS[i % len(UNOBSERVED_KINDS)]
        if kind == "flow nan":
            flow[m, n, l] = np.nan
        else:
            var[m, n, l] = {"var +inf": np.inf, "var nan": np.nan, "var 0": 0.0, "var -1": -1.0}[kind]
    return flow, var, mu0, sigma0


def observed(flow, var):
    with np.errstate(invalid="ignore"):
        return np.isfinite(flow) & np.isfinite(var) & (var > 0)


def scrub(flow, var):
    """Every unobserved entry rewritten in both fields: flow (a NaN, or whatever sat
    beside a bad variance) -> 1e300, var (-1, NaN, +Inf, 0, or a good one beside a NaN
    flow) -> 0.  The variance 0 keeps each of them unobserved; the observed entries keep
    their bits."""
    seen = observed(flow, var)
    f2, v2 = flow.copy(order="F"), var.copy(order="F")
    f2[~seen], v2[~seen] = 1e300, 0.0
    assert np.array_equal(observed(f2, v2), seen)
    return f2, v2
