"""The rounding problem of the CIA backend restated in numpy, three ways, and its test inputs.

``mpcx_cia_round`` (include/mpcx.h) rounds relaxed binary controls b[j][i] to B[j][i] in {0, 1}
with one 1 per interval so that eta = max_{j,k} |sum_{i<=k} dt (b - B)| is least.  Everything is
exact fp64 arithmetic (ascending running sums, single subtractions, compares), so the statements
below and the kernel agree bit for bit:

* :func:`enumerate_eta`  every one of the nc^N assignments (small sizes only);
* :func:`dp_full`        the recursion over count vectors as the header states it, every state kept;
* :func:`round_batch`    the same recursion restricted to the band of sum-up rounding, state for
  state what one lane of the kernel does, vectorised over agents -- the reference of the GPU tests.
"""

import itertools

import numpy as np

OK, BAD_INPUT, BAND_OVERFLOW = 0, 1, 2
MAX_MODES, MAX_INTERVALS, MAX_STATES = 4, 128, 64
CLIP_TOL, COL_TOL = 1e-5, 1e-6


def clip(v):
    """Values just outside [0, 1] onto the bounds, the way the reference does before rounding."""
    v = np.asarray(v, dtype=np.float64)
    v = np.where((v > -CLIP_TOL) & (v < 0.0), 0.0, v)
    return np.where((v > 1.0) & (v < 1.0 + CLIP_TOL), 1.0, v)


def modes(b_rel):
    """(b [A, nc, N], bad [A]): the clipped controls with the dummy mode of a single control, and
    which agents' input is unusable."""
    b = clip(b_rel)
    A, n_bin, N = b.shape
    with np.errstate(invalid="ignore"):
        bad = ~((b >= 0.0) & (b <= 1.0)).all(axis=(1, 2))
        if n_bin >= 2:
            s = b[:, 0, :]
            for r in range(1, n_bin):
                s = s + b[:, r, :]
            bad |= ~(np.abs(s - 1.0) <= COL_TOL).all(axis=1)
        else:
            b = np.concatenate([b, np.maximum(0.0, 1.0 - b)], axis=1)
    return b, bad


def running_sums(b):
    """S [nc, N]: plain adds in ascending i."""
    S = np.zeros_like(b)
    acc = np.zeros(b.shape[0])
    for i in range(b.shape[1]):
        acc = acc + b[:, i]
        S[:, i] = acc
    return S


def deviation(b, B):
    """max_{j,k} |S_j[k] - c_j[k]| of an assignment B [nc, N] (in intervals)."""
    S = running_sums(b)
    c = np.cumsum(np.asarray(B, dtype=np.int64), axis=1)
    return float(np.max(np.abs(S - c.astype(np.float64))))


def enumerate_eta(b, n_best=1):
    """The ``n_best`` smallest distinct deviations over all nc^N assignments, ascending."""
    nc, N = b.shape
    S = running_sums(b)
    found = set()
    for choice in itertools.product(range(nc), repeat=N):
        c = np.zeros(nc)
        e = 0.0
        for i, j in enumerate(choice):
            c[j] += 1.0
            e = max(e, float(np.max(np.abs(S[:, i] - c))))
        found.add(e)
    return sorted(found)[:n_best]


def dp_full(b):
    """(eta, B [nc, N]): F(i,c) = max(dev(i,c), min_j F(i-1, c-e_j)) over every count vector; the
    predecessor is the smallest j that attains the minimum, the final c the lexicographically
    smallest."""
    nc, N = b.shape
    S = running_sums(b)
    F = {(0,) * nc: 0.0}
    preds = []
    for i in range(N):
        G, P = {}, {}
        for c in sorted(F):
            for j in range(nc):
                c2 = c[:j] + (c[j] + 1,) + c[j + 1:]
                if c2 not in G:
                    G[c2] = None
        for c2 in G:
            best, bj = np.inf, 0
            for j in range(nc):
                c1 = c2[:j] + (c2[j] - 1,) + c2[j + 1:]
                if c2[j] >= 1 and c1 in F and F[c1] < best:
                    best, bj = F[c1], j
            dev = max(abs(S[k, i] - float(c2[k])) for k in range(nc))
            G[c2], P[c2] = max(dev, best), bj
        F = G
        preds.append(P)
    eta = min(F.values())
    c = min(c for c in F if F[c] == eta)
    B = np.zeros((nc, N))
    for i in range(N - 1, -1, -1):
        j = preds[i][c]
        B[j, i] = 1.0
        c = c[:j] + (c[j] - 1,) + c[j + 1:]
    return float(eta), B


def round_batch(b_rel, dt):
    """What ``mpcx_cia_round`` computes for relaxed controls ``b_rel`` [A, n_bin, N]: a dict of
    ``status`` [A] int32, ``eta`` [A] (dt applied last; NaN where not OK), ``b_bin`` [A, n_bin, N]
    (NaN where not OK) and ``eta_sur`` [A] (in intervals).  The band: W = floor(2 eta_sur) + 2
    counts per mode from ceil(S_j[i] - eta_sur) - 1 on, W^(nc-1) <= 64 states, state s the count
    vector whose digits (the first mode's most significant) are s in base W."""
    b_rel = np.asarray(b_rel, dtype=np.float64)
    A, n_bin, N = b_rel.shape
    assert 1 <= n_bin <= MAX_MODES and 1 <= N <= MAX_INTERVALS
    b, bad = modes(b_rel)
    nc = b.shape[1]
    nm = nc - 1
    b = np.where(bad[:, None, None], 1.0 / nc, b)  # anything valid: the result is masked below
    rows = np.arange(A)
    # sum-up rounding
    acc = np.zeros((A, nc))
    cs = np.zeros((A, nc), dtype=np.int64)
    eta = np.zeros(A)
    for i in range(N):
        acc = acc + b[:, :, i]
        js = np.argmax(acc - cs.astype(np.float64), axis=1)  # the first of equal maxima
        cs[rows, js] += 1
        eta = np.maximum(eta, np.max(np.abs(acc - cs.astype(np.float64)), axis=1))
    W = np.floor(2.0 * eta).astype(np.int64) + 2
    overflow = W ** nm > MAX_STATES
    W = np.where(overflow, 2, W)  # masked below
    slots = W ** nm
    s = np.arange(MAX_STATES)[None, :]
    stride = [W ** (nm - 1 - k) for k in range(nm)]
    digit = [(s // stride[k][:, None]) % W[:, None] for k in range(nm)]
    # the levels
    fprev = np.where(s == 0, 0.0, np.inf) * np.ones((A, 1))
    lo_prev = np.zeros((A, nm), dtype=np.int64)
    pred = np.zeros((A, N, MAX_STATES), dtype=np.int64)
    los = np.zeros((A, N, nm), dtype=np.int64)
    acc = np.zeros((A, nc))
    for i in range(N):
        acc = acc + b[:, :, i]
        lo = np.ceil(acc[:, :nm] - eta[:, None]).astype(np.int64) - 1
        overflow |= (np.abs(acc[:, :nm] - (lo + W[:, None]).astype(np.float64)) <= eta[:, None]).any(axis=1)
        c = [lo[:, k, None] + digit[k] for k in range(nm)]
        c.append(i + 1 - sum(c))
        valid = s < slots[:, None]
        for cj in c:
            valid = valid & (cj >= 0)
        dev = np.zeros((A, MAX_STATES))
        for j in range(nc):
            dev = np.maximum(dev, np.abs(acc[:, j, None] - c[j].astype(np.float64)))
        live = valid & (dev <= eta[:, None])
        best = np.full((A, MAX_STATES), np.inf)
        bj = np.zeros((A, MAX_STATES), dtype=np.int64)
        for j in range(nc):
            ok = c[j] >= 1
            sp = np.zeros((A, MAX_STATES), dtype=np.int64)
            for k in range(nm):
                dp = c[k] - (1 if k == j else 0) - lo_prev[:, k, None]
                ok = ok & (dp >= 0) & (dp < W[:, None])
                sp = sp + dp * stride[k][:, None]
            v = np.take_along_axis(fprev, np.where(ok, sp, 0), axis=1)
            better = ok & (v < best)
            best = np.where(better, v, best)
            bj = np.where(better, j, bj)
        fprev = np.where(live, np.maximum(dev, best), np.inf)
        pred[:, i, :] = bj
        los[:, i, :] = lo
        lo_prev = lo
    fmin = fprev.min(axis=1)
    overflow |= ~np.isfinite(fmin)
    state = np.argmax(fprev == fmin[:, None], axis=1)  # the smallest state that attains it
    # walk back
    c = np.stack([lo_prev[:, k] + (state // stride[k]) % W for k in range(nm)], axis=1)
    mode = np.zeros((A, N), dtype=np.int64)
    for i in range(N - 1, -1, -1):
        j = pred[rows, i, state % MAX_STATES]
        mode[:, i] = j
        for k in range(nm):
            c[:, k] -= (j == k)
        lo_before = los[:, i - 1, :] if i > 0 else np.zeros((A, nm), dtype=np.int64)
        state = sum((c[:, k] - lo_before[:, k]) * stride[k] for k in range(nm))
    okay = ~bad & ~overflow
    b_bin = (mode[:, None, :] == np.arange(n_bin)[None, :, None]).astype(np.float64)
    b_bin = np.where(okay[:, None, None], b_bin, np.nan)
    status = np.where(bad, BAD_INPUT, np.where(overflow, BAND_OVERFLOW, OK)).astype(np.int32)
    return {"status": status, "eta": np.where(okay, dt * fmin, np.nan), "b_bin": b_bin, "eta_sur": eta}


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def random_controls(rng, A, n_bin, N, kind="random"):
    """Relaxed controls [A, n_bin, N].  ``random``: uniform (one control) or Dirichlet columns,
    every other agent's concentrated near the corners; ``ties``: a quarter grid, which makes many
    assignments equally good; ``integral``: already binary."""
    if kind == "integral":
        pick = rng.integers(0, max(n_bin, 2), size=(A, N))
        return (pick[:, None, :] == np.arange(n_bin)[None, :, None]).astype(np.float64)
    if n_bin == 1:
        b = rng.random((A, 1, N))
        return np.round(b * 4.0) / 4.0 if kind == "ties" else b
    if kind == "ties":
        # quarters that sum to 4: n_bin - 1 sorted cuts of [0, 4]
        cuts = np.sort(rng.integers(0, 5, size=(A, n_bin - 1, N)), axis=1)
        edges = np.concatenate([np.zeros((A, 1, N), dtype=np.int64), cuts,
                                np.full((A, 1, N), 4, dtype=np.int64)], axis=1)
        return np.diff(edges, axis=1) / 4.0
    alpha = np.where(np.arange(A) % 2 == 1, 0.3, 1.0)[:, None, None] * np.ones((A, N, n_bin))
    g = rng.standard_gamma(alpha)
    g = g / g.sum(axis=2, keepdims=True)
    return np.ascontiguousarray(np.transpose(g, (0, 2, 1)))


def scattered_positions(rng, n_bin, N, nw):
    """Distinct positions [n_bin, N] of the binary controls in a row of nw entries, in no order."""
    return rng.permutation(nw)[:n_bin * N].reshape(n_bin, N)


# ---------------------------------------------------------------------------
# the on / off cooler room (benchmarks.one_room_cia) written out by hand
# ---------------------------------------------------------------------------
COOLER_MAX_POWER = 1000.0


def cooler_room(N=10, ts=300.0, d=2):
    """The NLP that backend ``casadi_cia`` transcribes from the cooler room with collocation, in
    torch (autograd derivatives), the way oracle/nlps.py states the other structures.

    w = [T_0, (P_k, b_k, (T, T_slack, T_out) per point, T_{k+1}) per interval],
    p = [T0, cp, C, s_T, r_cooling, cooler_mod_limit, (load, T_upper, T_in) per point],
    g = per interval [continuity, (collocation, P - 1000 b <= 0, P - limit b >= 0,
    0 <= T + T_slack <= T_upper, T_out - T = 0) per point]."""
    import torch

    from oracle import nlps

    tau, B, C, D = nlps.collocation(d, "legendre")
    nb = 2 + 3 * d + 1
    n = 1 + N * nb
    per = 1 + 5 * d
    m = N * per
    npg, nps = 6, 3 * d
    names = ["T@0"]
    for k in range(N):
        names += [f"cooling_power@{k}", f"cooler_on@{k}"]
        for j in range(d):
            names += [f"T@{k},{j}", f"T_slack@{k},{j}", f"T_out@{k},{j}"]
        names.append(f"T@{k + 1}")

    def f(w, p):
        s_T, r = p[3], p[4]
        tot = w.new_zeros(())
        for k in range(N):
            o = 1 + k * nb
            for j in range(d):
                tot = tot + B[j + 1] * (r * w[o] + s_T * w[o + 2 + 3 * j + 1] ** 2) * ts
        return tot

    def g(w, p):
        Cz, limit = p[2], p[5]
        out = []
        xk = w[0]
        for k in range(N):
            o = 1 + k * nb
            power, on = w[o], w[o + 1]
            Tj = [w[o + 2 + 3 * j] for j in range(d)]
            x_end = w[o + nb - 1]
            out.append(x_end - (D[0] * xk + sum(D[j + 1] * Tj[j] for j in range(d))))
            for j in range(d):
                load = p[npg + k * nps + 3 * j]
                xp = C[0, j + 1] * xk + sum(C[q + 1, j + 1] * Tj[q] for q in range(d))
                out.append(ts * ((load - power) / Cz) - xp)
                out.append(power - on * COOLER_MAX_POWER)
                out.append(power - on * limit)
                out.append(Tj[j] + w[o + 2 + 3 * j + 1])
                out.append(w[o + 2 + 3 * j + 2] - Tj[j])
            xk = x_end
        return torch.stack(out)

    def lbg(p):
        lb = np.zeros(m)
        for k in range(N):
            for j in range(d):
                lb[k * per + 1 + 5 * j + 1] = -np.inf
        return lb

    def ubg(p):
        ub = np.zeros(m)
        for k in range(N):
            for j in range(d):
                q = k * per + 1 + 5 * j
                ub[q + 2] = np.inf
                ub[q + 3] = p[npg + k * nps + 3 * j + 1]
        return ub

    return nlps.OracleProblem("cooler_room", n, m, npg + N * nps, f, g, lbg, ubg, names)


def cooler_room_inputs(prob, N=10, d=2, T0=298.16, load=150.0, T_in=290.15, T_upper=295.15, s_T=3.0,
                       r_cooling=1 / 3, cooler_mod_limit=250.0, cp=1000.0, C=100000.0):
    """(p, lbw, ubw, w0) of a cold start with the example's bounds; ``binary`` positions via
    :func:`cooler_room_binary_positions`."""
    p = np.array([T0, cp, C, s_T, r_cooling, cooler_mod_limit] + [load, T_upper, T_in] * (N * d), float)
    lbw = np.full(prob.n, -np.inf)
    ubw = np.full(prob.n, np.inf)
    w0 = np.zeros(prob.n)
    for i, name in enumerate(prob.w_names):
        base = name.split("@")[0]
        if base == "T":
            lbw[i], ubw[i], w0[i] = 288.15, 303.15, T0
        elif base == "cooling_power":
            lbw[i], ubw[i], w0[i] = 0.0, 500.0, 250.0
        elif base == "cooler_on":
            lbw[i], ubw[i], w0[i] = 0.0, 1.0, 0.5
    lbw[0] = ubw[0] = w0[0] = T0
    return p, lbw, ubw, w0


def cooler_room_binary_positions(prob):
    return np.array([[i for i, name in enumerate(prob.w_names) if name.startswith("cooler_on@")]])
