"""Extended-precision CPU reference of the diffuse field for several columns of illumination and the rows of LOS steps
(sr_diffuse_source_columns_dev, engine.diffuse_source_columns), its yardstick and the case set of
tests/test_diffuse_columns_host.py and tests/test_gpu_diffuse_columns.py.  A helper module: no fixture, no pytest
setting, nothing that needs a GPU.

reference        per column diffuse_source_reference.reference (long double) for (mu0[c], beam[c]), then the gather
                     rows[r] = ssa_G (1 - f_G) sca[src_row[r]] sum_c col_w[r, c] J[c, row_layer[r]]
                 in long double.
plain64_columns  the kernel's formulas as built, in fp64 numpy: the layer operators once, the sources from the two
                 shared factors (E+ + E- = D fs, E+ - E- = D mu0 fd), a column's two sweeps, the dense dot product with
                 c ascending from the first term, then (w_out sca) dot.

The yardstick, eps = 2^-53: b = R.bound(ref, n_gas, n_layers) for J and the fluxes, and b + eps n_col |ref| for the rows
(one rounding per term of the dot product on top of J's).

Cases: a case of diffuse_source_reference with C columns, column c given mu0 = linspace(-0.2, 0.8, C)[c] and
beam_c = beam ** (0.5 + 0.75 c / (C - 1)); for C == 1 the case's own values.
"""
import numpy as np

import diffuse_source_reference as R

LD = R.LD
EPS53 = R.EPS53
N_COL = (1, 2, 3, 5, 8)     # cycled over the GPU panel: 3 and 5 run padded instances


def columns_of(c, C):
    """(mu0s [C], beams [C, N + 1, n_pts]) of the case c with C columns."""
    if C == 1:
        return np.array([c["mu0"]]), np.ascontiguousarray(c["beam"][None])
    mu0s = np.linspace(-0.2, 0.8, C)
    beams = np.stack([c["beam"] ** (0.5 + 0.75 * k / (C - 1)) for k in range(C)])
    return mu0s, np.ascontiguousarray(beams)


def rows_of(rng, n_layers, C, n_src=None):
    """(col_w [n_rows, C], row_layer, src_row) of the GPU panel: n_rows = 2 n_layers + 3 in shuffled order, one layer
    without a row (n_layers > 1), one with three, one row with all-zero weights, one dense, the rest two adjacent
    non-zeros (one for C == 1); src_row a permutation into a table of n_src = n_layers + 1 rows."""
    n_rows = 2 * n_layers + 3
    n_src = n_layers + 1 if n_src is None else n_src
    if n_layers > 1:
        none, three = (int(x) for x in rng.choice(n_layers, 2, replace=False))
        others = [l for l in range(n_layers) if l not in (none, three)] or [three]   # (two layers: every row on one)
        layers = [l for l in range(n_layers) if l != none] * 2 + [three] + [int(rng.choice(others)) for _ in range(4)]
    else:
        layers = [0] * n_rows
    layers = np.array(layers, np.int32)
    assert layers.shape == (n_rows,)
    w = np.zeros((n_rows, C))
    for r in range(n_rows):
        if r == 1:
            continue                                    # all-zero weights
        if r == 0 or C == 1:
            w[r] = rng.uniform(0.1, 1.0, C)             # dense
        else:
            k = int(rng.integers(0, C - 1))
            t = rng.uniform()
            w[r, k], w[r, k + 1] = 1.0 - t, t
    order = rng.permutation(n_rows)
    w, layers = w[order], layers[order]
    src = (rng.permutation(max(n_src, n_rows))[:n_rows] % n_src).astype(np.int32)
    return w, layers, src


def reference(c, mu0s, beams, col_w=None, row_layer=None, sca=None, src_row=None):
    """dict(J [C, N, n_pts], flux [C, 2, N + 1, n_pts], rows [n_rows, n_pts] if col_w is given) in long double."""
    per = [R.reference(c["A"], c["V"], c["ssa"], c["asym"], beams[k], c["sun"], mu0s[k], c["albedo"], c["out_gas"])
           for k in range(len(mu0s))]
    out = dict(J=np.stack([p["J"] for p in per]), flux=np.stack([p["flux"] for p in per]))
    if col_w is not None:
        G = c["out_gas"]
        ssa, asym = np.asarray(c["ssa"], LD), np.asarray(c["asym"], LD)
        w_out = ssa[G] * (1 - R._f(asym, LD)[G])
        sca = np.asarray(c["A"][G] if sca is None else sca, LD)
        src_row = row_layer if src_row is None else src_row
        dot = np.einsum("rc,crj->rj", np.asarray(col_w, LD), out["J"][:, row_layer, :])
        out["rows"] = w_out * sca[src_row] * dot
    return out


def bounds(ref, n_gas, n_layers, n_col):
    b = {k: R.bound(ref[k], n_gas, n_layers) for k in ("J", "flux")}
    if "rows" in ref:
        b["rows"] = R.bound(ref["rows"], n_gas, n_layers) + LD(EPS53) * n_col * np.abs(ref["rows"])
    return b


def _shared_operators(sp, al, sg):
    """The kernel's diffuse_layer_shared in fp64: dict(R, T, oneR, absb, fs, fd, live) of one layer."""
    ft = np.float64
    dtau, live, co, om, g, d, s = R._coefficients(sp, al, sg, ft)
    r3 = ft(1.7320508075688772)
    d, s = r3 * co, r3 * (1.0 - om * g)
    sd, ss = np.sqrt(d), np.sqrt(s)
    k, g1 = sd * ss, 0.5 * (s + d)
    g2 = 0.5 * (r3 * om * (1.0 - g))
    rg = 1.0 / (g1 + k)
    Gm, u = g2 * rg, sd * (sd + ss) * rg
    x = k * dtau
    e, m = np.exp(-x), -np.expm1(-x)
    ge = 1.0 + Gm * e
    rden = 1.0 / ((u + Gm * m) * ge)
    Rr = Gm * m * (1.0 + e) * rden
    T = e * u * (1.0 + Gm) * rden
    oneR = u * (1.0 + Gm * e * e) * rden
    absb = m * u * (1.0 - Gm * e) * rden
    oneT = m * (u + Gm * ge) * rden
    fs = om * (sd + ss) * rg * (m / sd) / ge
    fd = -(om * (r3 * g)) / s * (oneT + Rr)
    o = dict(R=Rr, T=T, oneR=oneR, absb=absb, fs=fs, fd=fd)
    idle = dict(R=0.0, T=1.0, oneR=1.0, absb=0.0, fs=0.0, fd=0.0)
    o = {key: np.where(live, val, idle[key]) for key, val in o.items()}
    o["live"] = live
    return o


def plain64_columns(c, mu0s, beams, col_w=None, row_layer=None, sca=None, src_row=None):
    """The kernel's formulas term by term in fp64: the same dict."""
    with np.errstate(divide="ignore", invalid="ignore"):
        sp, al, sg = R.optics_kernel(c["A"], c["V"], c["ssa"], c["asym"])
        N, n_pts = sp.shape
        C = len(mu0s)
        sun, alb = np.asarray(c["sun"], np.float64), np.float64(c["albedo"])
        beams = np.asarray(beams, np.float64)
        Rb, Cb = np.full(n_pts, alb), np.full(n_pts, 1.0 - alb)
        Ub = [alb * (max(float(mu0s[k]), 0.0) * (sun * beams[k, N])) for k in range(C)]
        keep = []
        for l in range(N):
            o = _shared_operators(sp[l], al[l], sg[l])
            q = np.where(o["live"], 1.0 / (Cb + Rb * o["oneR"]), 1.0)
            cq, ub = [], []
            for k in range(C):
                D = sun * beams[k, l]
                es, ed = D * o["fs"], (D * np.float64(mu0s[k])) * o["fd"]
                Ep, Em = 0.5 * (es + ed), 0.5 * (es - ed)
                cq.append((Em + o["R"] * Ub[k]) * q)
                ub.append(Ub[k])
                Ub[k] = Ep + o["T"] * (Ub[k] + Rb * Em) * q
            keep.append((o["T"] * q, Rb, cq, ub))
            Cb = (o["oneR"] * Cb + Rb * o["absb"] * (o["oneR"] + o["T"])) * q
            Rb = o["R"] + o["T"] * o["T"] * Rb * q
        F = np.zeros((C, 2, N + 1, n_pts))
        J = np.zeros((C, N, n_pts))
        kJ = np.float64(1.7320508075688772) / (8.0 * 3.141592653589793)
        for k in range(C):
            F[k, 0, N] = Ub[k]
            for l in range(N - 1, -1, -1):
                tq, rb, cq, ub = keep[l]
                F[k, 1, l] = tq * F[k, 1, l + 1] + cq[k]
                F[k, 0, l] = ub[k] + rb * F[k, 1, l]
                J[k, l] = kJ * ((F[k, 0, l] + F[k, 1, l]) + (F[k, 0, l + 1] + F[k, 1, l + 1]))
    out = dict(J=J, flux=F)
    if col_w is not None:
        G = c["out_gas"]
        ssa, asym = np.asarray(c["ssa"], np.float64), np.asarray(c["asym"], np.float64)
        w_out = ssa[G] * (1.0 - R._f(asym, np.float64)[G])
        sca = np.asarray(c["A"][G] if sca is None else sca, np.float64)
        src_row = row_layer if src_row is None else src_row
        col_w = np.asarray(col_w, np.float64)
        rows = np.zeros((len(row_layer), n_pts))
        for r in range(len(row_layer)):
            dot = col_w[r, 0] * J[0, row_layer[r]]
            for k in range(1, C):
                dot = dot + col_w[r, k] * J[k, row_layer[r]]
            rows[r] = (w_out * sca[src_row[r]]) * dot
        out["rows"] = rows
    return out


def host_cases():
    """The case set of the host test: the GPU panel and the 300 random columns."""
    for n in R.N_LAYERS:
        for g in R.N_GAS:
            for p in R.N_PTS:
                yield R.panel_case(n, g, p)
    yield from R.random_columns()
