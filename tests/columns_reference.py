"""Extended-precision CPU reference of the Curtis-Godson columns (curgods.f:2-98: curgod_fort_1..4, the sums that
sr_los_columns_kernel and sr_curgod_kernel evaluate) and of the VMRs a retrieval's parameter vector gives at the sample
points (sr_los_vmr_from_params_kernel), in numpy.longdouble, with the yardstick of their error and the case set of
tests/test_columns_reference_host.py and tests/test_gpu_columns_reference.py.  A helper module: no fixture, no pytest
setting, nothing that needs a GPU.

The definition (curgod_fort_2, per step i -> i + 1 of a segment, summed in path order):

    dx = x1 - x0,  A = n0 v0,  B = n0 (v1 - v0) / dx,  fu = n1 / n0,  D = ln(fu) / dx
    col += (A D (fu - 1) + B fu (D dx - 1) + B) / D^2

The formula cancels where the density barely changes along a step (fu -> 1, D -> 0: the short segments of a tangent
shell): its three addends are each far larger than their sum.  That is the reference's own arithmetic (parity with
curgods.f is the requirement) and a RELATIVE tolerance means nothing there, so an error is counted in UNITS of

    2^-53 M + 1e-290,     M = sum over the steps of (|A D (fu - 1)| + |B fu (D dx - 1)| + |B|) / D^2

and likewise over the addends of the other three formulas (_terms).  M / |col| reaches 3e12 on the tangent segments of
the case set (n_sub = 32, 1e-9 km below a level) and stays at 1 to 3 elsewhere.  A segment of one sample point has
column 0 and M = 0: an exact 0.0 is expected (the absolute floor only lets results below the smallest normal double
count as zero).

columns_stable is the same integral, n0 e^(D t) (v0 + b t) over the step, in a form without the cancellation; the host
test holds columns(2) in long double to it, so the reference is not wrong where it matters most.

Equal densities at neighbouring sample points are 0 / 0 in curgods.f, in this module and in the kernels alike: no case
contains them (pool() asserts it) and no test feeds them, or a zero step length, to the device.
"""
import functools

import numpy as np

import pointing_reference as PR

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "numpy.longdouble is not an extended-precision type here: no reference, no fallback"

EPS53 = 2.0 ** -53
FLOOR = 1e-290
KERNEL_MARGIN = 8.0   # fused multiply-adds or none, another libm log, the order of the sum

# K_PLAIN: max over the case set of units(plain fp64, long double) -- columns(which, dtype=np.float64) against
# columns(which, dtype=LD) on the same fp64 inputs, in units of 2^-53 M.  The device's limit is KERNEL_MARGIN x the
# figure measured on a test's own inputs (k_plain), never one taken from the code under test.  Measured 2026-10-20 on
# the CPU over pool(n_sub) for n_sub in N_SUBS, all nine profiles (measure_k_plain):
#   which = 1: 1.22   which = 2: 3.88   which = 3: 2.66   which = 4: 4.01
# and for the parameter chain (vmr_from_params, then columns(2) of its rows, in the units of chain) over N_PARS:
#   VMRs 1.62, columns 2.25.
# Recorded at 1.5 x the measurement (the rule of limb_reference.py:33-39); tests/test_columns_reference_host.py asserts
# that the live measurement does not exceed them.
K_PLAIN_MEASURED = {1: 1.22, 2: 3.88, 3: 2.66, 4: 4.01}
K_PLAIN = {1: 1.9, 2: 5.9, 3: 4.0, 4: 6.1}
K_PLAIN_VMR_MEASURED, K_PLAIN_CHAIN_MEASURED = 1.62, 2.25
K_PLAIN_VMR, K_PLAIN_CHAIN = 2.4, 3.4

# the case set
N_SUBS = (1, 2, 3, 8, 32)
NEAR_LEVEL = 250.0                       # LEVELS[3] of pointing_reference
NEAR_OFFSETS = (1e-3, 1e-6, 1e-9)        # km from that level, on either side
Z_TANS = tuple(NEAR_LEVEL + sgn * d for d in NEAR_OFFSETS[::-1] for sgn in (-1.0, 1.0)) + PR.Z_TANS
N_PROF = 9                               # case_profiles' four, one identically 0, four more (the eight-gas batches)
ZERO_PROF = 4
RAGGED = (1, 2, 3, 4, 9, 33)             # sample points per segment of the ragged batch
SEG_COUNTS = ((1,), (63,), (64,), (65,), (130,), (1, 64, 65))   # segments per ray: 64 threads per block; 1 and 3 rays
N_PARS = (31, 32, 33, 65)                # parameters of the retrieval cases: kVmrParArg = 32 per block of kernel arguments


def profiles():
    """(z, nd [n_lev], vmr [N_PROF, n_lev]) on pointing_reference's levels.  No profile but the zero one is constant
    over a shell: with B = 0 the D error of the A addend alone, A dx / (D dx) against M = A dx, is no rounding matter."""
    z, nd, vmr = PR.case_profiles()
    more = np.array([1e-6 * np.exp((z - 100.0) / 80.0), 0.5 - 1e-3 * (z - 100.0), 2e-4 * (1.0 + 0.3 * np.sin(z / 40.0)),
                     7e-2 * (z / 100.0) ** -1.5])
    return z, nd, np.concatenate([vmr, np.zeros((1, z.size)), more])


@functools.lru_cache(maxsize=None)
def pool(n_sub):
    """Every segment of the case set's rays at n_sub, geometry_ld rounded to fp64 (the inputs of a plain implementation
    and of the kernels, taken as exact by the reference): x, nd, alt [n_seg, n_sub + 1], vmr [N_PROF, n_seg, n_sub + 1],
    ray [n_seg] (index into Z_TANS).  The near-level rays come first; 138 segments at every n_sub."""
    z, nd, vmr = profiles()
    out = dict(x=[], nd=[], alt=[], vmr=[], ray=[])
    for r, zt in enumerate(Z_TANS):
        G = PR.geometry_ld(z, nd, vmr, zt, n_sub=n_sub)
        for key in ("x", "nd", "alt"):
            out[key].append(np.asarray(G[key], np.float64))
        out["vmr"].append(np.asarray(G["vmr"], np.float64))
        out["ray"].append(np.full(len(G["k"]), r))
    P = dict(x=np.concatenate(out["x"]), nd=np.concatenate(out["nd"]), alt=np.concatenate(out["alt"]),
             vmr=np.concatenate(out["vmr"], axis=1), ray=np.concatenate(out["ray"]))
    assert np.all(np.diff(P["nd"], axis=1) != 0.0) and np.all(np.diff(P["x"], axis=1) > 0.0), "0 / 0 in the case set"
    for v in P.values():
        v.setflags(write=False)
    return P


def batch(n_sub, seg_counts, start=0, points=None):
    """A LOS batch of the case set in fp64: rays of seg_counts segments taken from pool(n_sub) in order, from segment
    `start` on (wrapping round); points: sample points per segment (the first of each pool segment; None: all n_sub + 1).
    seg_layer = arange per ray (every segment on a row of its own: the read-out of the GPU tests).  Returns seg_off,
    seg_layer, pt_off, x, nd, alt [n_pt], vmr [N_PROF, n_pt]."""
    P = pool(n_sub)
    n_seg = int(np.sum(seg_counts))
    segs = (start + np.arange(n_seg)) % P["x"].shape[0]
    npts = np.full(n_seg, n_sub + 1) if points is None else np.asarray(points)
    assert npts.size == n_seg and npts.max() <= n_sub + 1
    take = np.concatenate([s * (n_sub + 1) + np.arange(k) for s, k in zip(segs, npts)])
    flat = lambda a: np.ascontiguousarray(a.reshape(a.shape[:-2] + (-1,))[..., take])
    return dict(seg_off=np.concatenate([[0], np.cumsum(seg_counts)]).astype(np.int32),
                seg_layer=np.concatenate([np.arange(k) for k in seg_counts]).astype(np.int32),
                pt_off=np.concatenate([[0], np.cumsum(npts)]).astype(np.int32),
                x=flat(P["x"]), nd=flat(P["nd"]), alt=flat(P["alt"]), vmr=flat(P["vmr"]))


def tangent_start(n_sub):
    """The pool index of the far-side tangent segment of the first ray (1e-9 km below a level: the shortest segment)."""
    P = pool(n_sub)
    first = np.flatnonzero(P["ray"] == 0)
    return int(first[len(first) // 2 - 1])


# ------------------------------------------------------------------------------------------------------------------
# the sums
# ------------------------------------------------------------------------------------------------------------------
def _terms(which, dx, n0, n1, v0, v1, f0, f1, dtype):
    """(the step's term, the sum of its absolute addends) of curgod_fort_`which` in `dtype`, the operations of
    curgods.f in their order.  v0, v1 may carry leading axes (profiles)."""
    one, two = dtype(1), dtype(2)
    if which == 1:
        fu = n1 / n0
        D = np.log(fu) / dx
        return (n1 - n0) / D, (np.abs(n1) + np.abs(n0)) / np.abs(D)
    if which in (2, 4):
        if which == 2:
            A = n0 * v0
            B = n0 * (v1 - v0) / dx
            fu = n1 / n0
        else:
            A = n0 * v0 * f0
            B = n0 * f0 * ((v1 - v0) / dx)
            fu = n1 * f1 / (n0 * f0)
        D = np.log(fu) / dx
        a1, a2 = A * D * (fu - one), B * fu * (D * dx - one)
        return (a1 + a2 + B) / (D * D), (np.abs(a1) + np.abs(a2) + np.abs(B)) / (D * D)
    A = n0 * v0 * f0
    cc = (v1 - v0) / dx
    bb = (f1 - f0) / dx
    B = n0 * (v0 * bb + f0 * cc)
    C = n0 * bb * cc
    fu = n1 / n0
    D = np.log(fu) / dx
    L = D * dx
    val = (fu * (D * (A * D + B * (L - one)) + C * (L * (L - two) + two)) + D * (B - A * D) - two * C) / (D * D * D)
    M = (np.abs(fu * A * D * D) + np.abs(fu * B * D * (L - one)) + np.abs(fu * C * L * (L - two)) + np.abs(two * fu * C)
         + np.abs(D * B) + np.abs(A * D * D) + np.abs(two * C)) / np.abs(D * D * D)
    return val, M


def columns(which, x, nd, vmr=None, f=None, pt_off=None, dtype=LD, scale=None):
    """(col, M) of curgod_fort_`which` (1..4) over ragged segments: segment s owns the sample points
    pt_off[s]:pt_off[s + 1] of x, nd, f [n_pt] and vmr [n_pt] or [n_prof, n_pt] (one column row per profile); pt_off
    None: one segment.  Evaluated in `dtype`, the steps added in path order from 0; M as in the module docstring.
    scale [n_prof]: col_scale, one more product in `dtype` (M takes |scale|).  Returns [n_seg] or [n_prof, n_seg]."""
    assert which in (1, 2, 3, 4)
    x, nd = np.asarray(x, dtype), np.asarray(nd, dtype)
    pt_off = np.array([0, x.size]) if pt_off is None else np.asarray(pt_off, np.int64)
    n_seg = pt_off.size - 1
    v = np.zeros((1, x.size), dtype) if which == 1 else np.atleast_2d(np.asarray(vmr, dtype))
    ff = np.ones(x.size, dtype) if which < 3 else np.asarray(f, dtype)
    col, M = np.zeros((v.shape[0], n_seg), dtype), np.zeros((v.shape[0], n_seg), dtype)
    for k in range(int(np.max(np.diff(pt_off))) - 1 if n_seg else 0):
        segs = np.flatnonzero(pt_off[:-1] + k + 1 < pt_off[1:])
        i = pt_off[segs] + k
        t, m = _terms(which, x[i + 1] - x[i], nd[i], nd[i + 1], v[:, i], v[:, i + 1], ff[i], ff[i + 1], dtype)
        col[:, segs] = col[:, segs] + t
        M[:, segs] = M[:, segs] + m
    if scale is not None:
        sc = np.asarray(scale, dtype).reshape(-1, 1)
        col, M = sc * col, np.abs(sc) * M
    one_row = which == 1 or np.ndim(vmr) == 1
    return (col[0], M[0]) if one_row else (col, M)


def columns_stable(x, nd, vmr, pt_off=None):
    """curgod_fort_2's integral in long double without its cancellation: per step, with d = (n1 - n0) / n0 (exact to a
    rounding), L = log1p(d) and b = v1 - v0,
        n0 dx (v0 d / L + b psi(L)),     psi(L) = int_0^1 s e^(L s) ds = (L (1 + d) - d) / L^2,
    psi by its series sum_k L^k / (k! (k + 2)) below |L| = 0.5.  Linear in vmr with non-negative weights: of a
    non-negative `vmr` it is also the bound of what errors of that size at the sample points do to a column."""
    x, nd = np.asarray(x, LD), np.asarray(nd, LD)
    v = np.atleast_2d(np.asarray(vmr, LD))
    pt_off = np.array([0, x.size]) if pt_off is None else np.asarray(pt_off, np.int64)
    i = np.concatenate([np.arange(a, b - 1) for a, b in zip(pt_off[:-1], pt_off[1:])] + [np.zeros(0, np.int64)]).astype(np.int64)
    seg = np.concatenate([np.full(max(b - 1 - a, 0), s) for s, (a, b) in enumerate(zip(pt_off[:-1], pt_off[1:]))] + [np.zeros(0, np.int64)])
    d = (nd[i + 1] - nd[i]) / nd[i]
    L = np.log1p(d)
    small = np.abs(L) < 0.5
    Ls = np.where(small, L, LD(0))
    psi_s, term = np.zeros_like(L), np.ones_like(L)          # term = L^k / k!
    for k in range(40):
        psi_s = psi_s + term / LD(k + 2)
        term = term * Ls / LD(k + 1)
    Lb = np.where(small, LD(1), L)
    psi = np.where(small, psi_s, (Lb * (LD(1) + d) - d) / (Lb * Lb))
    step = nd[i] * (x[i + 1] - x[i]) * (v[:, i] * (d / L) + (v[:, i + 1] - v[:, i]) * psi)
    col = np.zeros((v.shape[0], pt_off.size - 1), LD)
    for s in range(pt_off.size - 1):
        col[:, s] = step[:, seg == s].sum(axis=1)
    return col[0] if np.ndim(vmr) == 1 else col


def vmr_from_params(vmr, par_gas, par_w, x, dtype=LD):
    """(prof, Mv) [n_gas, n_pt]: prof[g] = sum_p [par_gas[p] == g] x_p par_w[p], added in the order of p from 0, in
    `dtype`; gases without parameters keep their row of vmr (Mv = 0: bit for bit).  Mv = sum_p |x_p par_w[p]|: errors of
    the VMRs are counted in units of 2^-53 Mv."""
    prof = np.array(np.atleast_2d(vmr), dtype)
    Mv = np.zeros(prof.shape, dtype)
    par_gas = np.asarray(par_gas)
    pw, xx = np.asarray(par_w, dtype), np.asarray(x, dtype)
    for g in np.unique(par_gas):
        prof[g] = 0
    for p, g in enumerate(par_gas):
        t = xx[p] * pw[p]
        prof[g] = prof[g] + t
        Mv[g] = Mv[g] + np.abs(t)
    return prof, Mv


def chain(b, par_gas, par_w, x, scale, dtype=LD):
    """Parameter vector -> VMRs -> columns of the gases, as sr_retrieval_forward_dev chains them on the batch `b` (its
    first len(scale) profiles are the gases).  Returns (prof, Mv, col, M): M = columns' own M + columns_stable(Mv), the
    second term being what errors of 2^-53 Mv in the VMRs do to a column, so that units of 2^-53 M hold both steps."""
    n_gas = len(scale)
    prof, Mv = vmr_from_params(b["vmr"][:n_gas], par_gas, par_w, x, dtype)
    col, M = columns(2, b["x"], b["nd"], prof, pt_off=b["pt_off"], dtype=dtype, scale=scale)
    M = M + np.abs(np.asarray(scale, LD))[:, None] * columns_stable(b["x"], b["nd"], np.asarray(Mv, LD), b["pt_off"])
    return prof, Mv, col, M


def mask_columns(b, par_gas, par_w, scale, dtype=LD):
    """(col, M) [n_par, n_seg] of the parameters' weight rows: scale[par_gas[p]] curgod_fort_2(nd, par_w[p], x)."""
    return columns(2, b["x"], b["nd"], par_w, pt_off=b["pt_off"], dtype=dtype, scale=np.asarray(scale)[np.asarray(par_gas)])


def units(got, ref, M):
    """|got - ref| / (2^-53 M + 1e-290), as fp64; a NaN or Inf in `got` is an error."""
    got = np.asarray(got)
    assert np.all(np.isfinite(np.asarray(got, np.float64))), "non-finite result"
    with np.errstate(under="ignore"):
        u = np.abs(np.asarray(got, LD) - np.asarray(ref, LD)) / (LD(EPS53) * np.asarray(M, LD) + LD(FLOOR))
    return np.asarray(u, np.float64)


def k_plain(which, x, nd, vmr=None, f=None, pt_off=None, scale=None):
    """max units(columns in np.float64, columns in long double) on these inputs: the yardstick of the device's limit."""
    ref, M = columns(which, x, nd, vmr, f, pt_off, LD, scale)
    got, _ = columns(which, x, nd, vmr, f, pt_off, np.float64, scale)
    return float(units(got, ref, M).max())


def k_plain_chain(b, par_gas, par_w, x, scale):
    """(VMRs, columns): max units of the plain fp64 chain against the long double one on these inputs."""
    prof, Mv, col, M = chain(b, par_gas, par_w, x, scale, LD)
    prof64, _, col64, _ = chain(b, par_gas, par_w, x, scale, np.float64)
    return float(units(prof64, prof, Mv).max()), float(units(col64, col, M).max())


# ------------------------------------------------------------------------------------------------------------------
# the parameters of the retrieval cases
# ------------------------------------------------------------------------------------------------------------------
BLOCK = 32   # kVmrParArg


def retrieval_par_gas(n_par):
    """par_gas [n_par] over four gases: gas 0 has parameters in the first block of 32 only, gas 1 only beyond index 32
    (33, 35 .. 63: its row starts in a later block), gas 2 on both sides of every block edge (.. 29, 31 | 32, 34 .. 62 |
    64: a later block adds to the row an earlier one started; at n_par = 33 the second block is that one addition),
    gas 3 none.  Up to 32 parameters gas 1 has none either."""
    p = np.arange(n_par)
    first = np.where((p % 3 == 2) | (p == BLOCK - 1), 2, 0)
    later = np.where(p % 2 == 0, 2, 1)
    return np.where(p < BLOCK, first, later).astype(np.int32)


def hat_weights(par_gas, alt, zero_rows=()):
    """par_w [n_par, n_pt]: the parameters of a gas are hat functions of altitude on nodes of their own between 100 and
    550 km (no plateau but 0: see profiles); zero_rows: parameters whose weights are all zero."""
    par_gas, alt = np.asarray(par_gas), np.asarray(alt, np.float64)
    W = np.zeros((par_gas.size, alt.size))
    for g in np.unique(par_gas):
        mine = np.flatnonzero(par_gas == g)
        nodes = np.linspace(100.0, 550.0, mine.size + 2)
        for c, p in zip(nodes[1:-1], mine):
            W[p] = np.clip(1.0 - np.abs(alt - c) / (nodes[1] - nodes[0]), 0.0, None)
    W[list(zero_rows)] = 0.0
    return W


def retrieval_x(par_gas, seed):
    """A parameter vector: VMR-like magnitudes per gas, every value with a factor of its own."""
    rng = np.random.default_rng([20261020, seed])
    return np.array([3e-1, 2e-2, 1e-1, 5e-3])[np.asarray(par_gas)] * rng.uniform(0.5, 1.5, len(par_gas))


RETRIEVAL_SCALE = (0.98827, 1.0, 0.5, 2.0)   # col_scale of the four gases


def measure_k_plain():
    """({which: K_PLAIN}, K_PLAIN_VMR, K_PLAIN_CHAIN) of the case set, live."""
    k = {w: 0.0 for w in (1, 2, 3, 4)}
    for n_sub in N_SUBS:
        P = pool(n_sub)
        n_seg = P["x"].shape[0]
        b = batch(n_sub, (n_seg,))
        for w in k:
            k[w] = max(k[w], k_plain(w, b["x"], b["nd"], b["vmr"], b["vmr"][2], b["pt_off"]))
    kv = kc = 0.0
    b = batch(3, (1, 64, 65))
    for n_par in N_PARS:
        pg = retrieval_par_gas(n_par)
        W = hat_weights(pg, b["alt"])
        for seed in (1, 2):
            a, c = k_plain_chain(b, pg, W, retrieval_x(pg, seed), RETRIEVAL_SCALE)
            kv, kc = max(kv, a), max(kc, c)
    return k, kv, kc
