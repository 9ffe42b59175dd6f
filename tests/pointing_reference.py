"""Extended-precision CPU reference of the pointing derivative's geometry (include/spectrobot_hip.h, sr_los_path and
sr_los_columns_dz): one limb ray through spherical shells rebuilt from the levels in numpy.longdouble -- crossings, sample
points, number density, VMRs -- the analytic derivatives of the sample points' path coordinate and altitude to the ray's
tangent altitude z_t with the crossed shells held fixed, and the forward-mode derivative of the Curtis-Godson sum
(curgod_fort_2, curgods.f:24-45) of every segment.  A plain fp64 restatement of that derivative is the yardstick of the
kernel's limit.  A helper module: no fixture, no pytest setting, nothing that needs a GPU.

The definition.  r_t = R + z_t; a shell [lo, hi] is crossed if hi > r_t, the tangent shell is the one with lo <= r_t.
Segment ends (km from the tangent point): s_hi = sqrt(hi^2 - r_t^2), d s_hi / d z_t = -r_t / s_hi; s_lo likewise where
lo > r_t, else 0 with derivative 0; mirrored on the far side.  Sample point i of [a, b]: s_i = a + (b - a) i / n_sub and
the same blend of the ends' derivatives; x_i = 1e5 s_i; alt_i = sqrt(s_i^2 + r_t^2) - R, d alt_i / d z_t =
(s_i d s_i + r_t) / (alt_i + R).  ln nd and every VMR are linear in altitude inside a segment:
d nd_i = nd_i slope_ln_nd d alt_i, d vmr_i = slope_vmr d alt_i, the slopes from the segment's first and last point.

Distances are per gas, relative to the largest |d col_g[s]| over the segments of the ray.
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "numpy.longdouble is not an extended-precision type here: no reference, no fallback"

# the case set
R_KM = 2575.0
N_SUB = 3
LEVELS = np.linspace(100.0, 500.0, 9)
Z_TANS = (127.3, 150.01, 260.0, 349.0, 470.0)   # mid-shell, just above a level, mid-shell, 1 km below a level, top shell
N_GAS_MAX = 4
ND_100 = 6.5e11                                  # cm^-3 at 100 km: coefficients of 1e-17 cm^2 then give optical depths of ~30


def diff_step(zt):
    """The step of the central differences of a ray: 1e-3 km, 1e-4 km for the stiff ray 1 km below a level."""
    return 1e-4 if float(zt) == 349.0 else 1e-3


def case_profiles(n_gas=N_GAS_MAX):
    """(z, nd [n_lev], vmr [n_gas, n_lev]) of the case set: a 45 km scale height with a 5 % ripple, smooth VMRs."""
    z = LEVELS
    nd = ND_100 * np.exp(-(z - 100.0) / 45.0) * (1.0 + 0.05 * np.sin(z / 23.0))
    vmr = np.array([0.3 * np.exp(-(z - 100.0) / 300.0), 0.02 + 1e-4 * (z - 100.0), 0.1 * (1.0 + 0.5 * np.cos(z / 90.0)),
                    5e-3 * (1.0 + ((z - 300.0) / 250.0) ** 2)])
    return z, nd, vmr[:n_gas]


# K_PLAIN_DCOL: max over the case set (five rays, four gases) of dist(plain fp64, reference): the plain fp64 forward-mode
# derivative (dcol_forward in np.float64) on the reference's geometry rounded to fp64, against the long double derivative
# on the unrounded geometry.  The kernel's limit is 8 x the yardstick's distance on a test's own inputs.  Measured
# 2026-10-19 on the CPU: 7.2e-15 (ray 349.0 km, gas 2: the ray 1 km below a level, where d x / d z_t is at its steepest
# and the rounding of x and of d x weighs most; the other four rays stay below 5e-16).  Recorded at 1.5 x the measurement
# (the rule of limb_reference.py:33-39); tests/test_pointing_reference_host.py asserts that the live measurement does not
# exceed it.
K_PLAIN_DCOL_MEASURED = 7.2e-15
K_PLAIN_DCOL = 1.1e-14
KERNEL_MARGIN = 8.0   # fused multiply-adds or none, another libm log, the sum's order

# the first step of the Richardson extrapolation of a ray (richardson): large enough for the truncation term to stand
# above the long double rounding of the differences where the ray allows it -- 150.01 km must stay above its level, 349.0 km
# below the next one
RICHARDSON_STEP = {127.3: 0.2, 150.01: 0.008, 260.0: 0.2, 349.0: 0.004, 470.0: 0.2}


def _profiles_ld(z, nd_levels, vmr_levels):
    """geometry._profiles in long double: the levels continued to the top boundary (one more shell of the last thickness)
    with the last scale height and the last VMR: (zz, ln nd, vmr) on the len(z) + 1 boundaries."""
    z = np.asarray(z, LD)
    ln = np.log(np.asarray(nd_levels, LD))
    vv = np.atleast_2d(np.asarray(vmr_levels, LD))
    top = z[-1] + (z[-1] - z[-2])
    ln_top = ln[-1] + (ln[-1] - ln[-2]) / (z[-1] - z[-2]) * (top - z[-1])
    return np.concatenate([z, [top]]), np.concatenate([ln, [ln_top]]), np.concatenate([vv, vv[:, -1:]], axis=1)


def crossed_shells(z, zt, R=R_KM):
    """The shells a ray at z_t crosses, by the rule of geometry._limb_crossings on its fp64 operands: hi > r_t."""
    z = np.asarray(z, float)
    zz = np.concatenate([z, [z[-1] + (z[-1] - z[-2])]])
    return np.nonzero(R + zz[1:] > R + float(zt))[0]


def geometry_ld(z, nd_levels, vmr_levels, zt, R=R_KM, n_sub=N_SUB, shells=None):
    """One limb ray in long double, photon order (far side, then near side).  z, nd_levels, vmr_levels, R: fp64 inputs
    taken as exact; zt may be long double (the differences move it).  shells: the crossed shells, held fixed (None:
    crossed_shells(zt)).  Returns k [n_seg], s [km], x [cm], alt [km], nd [n_seg, n_sub + 1], vmr [n_gas, n_seg,
    n_sub + 1] and the derivatives to z_t: ds, dx [cm / km], dalt."""
    zz, ln, vv = _profiles_ld(z, nd_levels, vmr_levels)
    R, zt = LD(R), LD(zt)
    rt = R + zt
    k = crossed_shells(z, float(zt), float(R)) if shells is None else np.asarray(shells)
    hi, lo = zz[k + 1], zz[k]
    above = (R + lo) > rt
    assert np.all(R + hi > rt) and np.count_nonzero(~above) == 1, "the shells are not those of this tangent altitude"
    s_hi = np.sqrt((hi - zt) * (R + hi + rt))
    s_lo = np.where(above, np.sqrt(np.where(above, (lo - zt) * (R + lo + rt), LD(0))), LD(0))
    d_hi = -rt / s_hi
    d_lo = np.where(above, -rt / np.where(above, s_lo, LD(1)), LD(0))
    kk = np.concatenate([k[::-1], k])
    a = np.concatenate([-s_hi[::-1], s_lo])[:, None]
    b = np.concatenate([-s_lo[::-1], s_hi])[:, None]
    da = np.concatenate([-d_hi[::-1], d_lo])[:, None]
    db = np.concatenate([-d_lo[::-1], d_hi])[:, None]
    i = np.arange(n_sub + 1).astype(LD)[None, :]
    f, g = i / LD(n_sub), (LD(n_sub) - i) / LD(n_sub)
    s, ds = a * g + b * f, da * g + db * f
    radius = np.sqrt(s * s + rt * rt)
    alt = radius - R
    # (s ds + r_t) without its cancellation: a da = b db = -r_t above the tangent shell, one end at rest inside it
    tangent = np.concatenate([~above[::-1], ~above])[:, None]
    far = (np.arange(2 * len(k)) < len(k))[:, None]
    num = np.where(tangent, np.where(far, rt * f * (LD(1) + g), rt * g * (LD(1) + f)),
                   -rt * f * g * (b - a) ** 2 / np.where(tangent, LD(1), a * b))
    dalt = num / radius
    w = ((alt - zz[kk][:, None]) / (zz[kk + 1] - zz[kk])[:, None])
    nd = np.exp(ln[kk][:, None] + (ln[kk + 1] - ln[kk])[:, None] * w)
    vmr = vv[:, kk][:, :, None] + (vv[:, kk + 1] - vv[:, kk])[:, :, None] * w[None]
    return dict(k=kk.astype(np.int32), s=s, x=s * LD(1e5), alt=alt, nd=nd, vmr=vmr, ds=ds, dx=ds * LD(1e5), dalt=dalt)


def columns(x, nd, vmr, dtype=LD):
    """curgod_fort_2 of every segment, [n_gas, n_seg], in `dtype` (no col_scale)."""
    x, nd, vmr = np.asarray(x, dtype), np.asarray(nd, dtype), np.asarray(vmr, dtype)
    one = dtype(1)
    acc = np.zeros(vmr.shape[:2], dtype)
    for i in range(x.shape[1] - 1):
        dx = x[:, i + 1] - x[:, i]
        A = nd[:, i] * vmr[:, :, i]
        B = nd[:, i] * (vmr[:, :, i + 1] - vmr[:, :, i]) / dx
        fu = nd[:, i + 1] / nd[:, i]
        D = np.log(fu) / dx
        acc = acc + (A * D * (fu - one) + B * fu * (D * dx - one) + B) / (D * D)
    return acc


def dcol_forward(x, nd, vmr, alt, dx_dz, dalt_dz, dtype=LD):
    """d col_g[s] / d z_t, [n_gas, n_seg], in `dtype`: the forward-mode derivative of `columns` term by term, its inputs
    d x from the path and d nd, d vmr from the segment's slopes (zero where its first and last altitude coincide).
    dtype long double on geometry_ld's arrays: the reference; np.float64 on fp64 arrays: the yardstick, the operations a
    plain implementation performs (sr_los_columns_dz_kernel's, in its order)."""
    x, nd, vmr, alt, dxz, daz = (np.asarray(v, dtype) for v in (x, nd, vmr, alt, dx_dz, dalt_dz))
    one, two, zero = dtype(1), dtype(2), dtype(0)
    dal = alt[:, -1] - alt[:, 0]
    flat = dal == zero
    safe = np.where(flat, one, dal)
    sl_nd = np.where(flat, zero, np.log(nd[:, -1] / nd[:, 0]) / safe)
    sl_v = np.where(flat, zero, (vmr[:, :, -1] - vmr[:, :, 0]) / safe)
    acc = np.zeros(vmr.shape[:2], dtype)
    for i in range(x.shape[1] - 1):
        dx, ddx = x[:, i + 1] - x[:, i], dxz[:, i + 1] - dxz[:, i]
        n0, n1, v0, v1 = nd[:, i], nd[:, i + 1], vmr[:, :, i], vmr[:, :, i + 1]
        dn0, dn1 = n0 * sl_nd * daz[:, i], n1 * sl_nd * daz[:, i + 1]
        dv0, dv1 = sl_v * daz[:, i], sl_v * daz[:, i + 1]
        A, dA = n0 * v0, dn0 * v0 + n0 * dv0
        B = n0 * (v1 - v0) / dx
        dB = (dn0 * (v1 - v0) + n0 * (dv1 - dv0)) / dx - B * ddx / dx
        fu = n1 / n0
        dfu = (dn1 - fu * dn0) / n0
        L, dL = np.log(fu), dfu / fu
        D = L / dx
        dD = (dL - D * ddx) / dx
        N = A * D * (fu - one) + B * fu * (L - one) + B
        dN = (dA * D * (fu - one) + A * dD * (fu - one) + A * D * dfu + dB * fu * (L - one) + B * dfu * (L - one)
              + B * fu * dL + dB)
        T = N / (D * D)
        acc = acc + (dN - two * T * D * dD) / (D * D)
    return acc


def dist(got, ref):
    """[n_gas]: max_s |got - ref| / max_s |ref| per gas, as fp64; a NaN or Inf in `got` is an error."""
    got = np.asarray(got)
    assert np.all(np.isfinite(np.asarray(got, np.float64))), "non-finite derivative"
    ref = np.asarray(ref, LD)
    return np.asarray(np.abs(np.asarray(got, LD) - ref).max(axis=1) / np.abs(ref).max(axis=1), np.float64)


def ray_case(zt, n_gas=N_GAS_MAX, shells=None):
    """One ray of the case set: (the long double geometry, the same arrays rounded to fp64 -- the inputs of a plain
    fp64 implementation and of the kernel)."""
    z, nd, vmr = case_profiles(n_gas)
    G = geometry_ld(z, nd, vmr, zt, shells=shells)
    return G, {key: np.asarray(G[key], np.float64) for key in ("x", "alt", "nd", "vmr", "dx", "dalt")}


def batch_inputs(z_tans=Z_TANS, n_gas=N_GAS_MAX):
    """The case set as one LOS batch in fp64 (engine.LimbLOS arguments + path) and the rays' long double geometry."""
    rays = [ray_case(zt, n_gas) for zt in z_tans]
    n_seg = [len(G["k"]) for G, _ in rays]
    cat = lambda key: np.concatenate([F[key].reshape(-1) for _, F in rays])
    los = dict(seg_off=np.concatenate([[0], np.cumsum(n_seg)]).astype(np.int32),
               seg_layer=np.concatenate([G["k"] for G, _ in rays]).astype(np.int32),
               pt_off=(np.arange(sum(n_seg) + 1) * (N_SUB + 1)).astype(np.int32), x=cat("x"), nd=cat("nd"),
               vmr=np.concatenate([F["vmr"].reshape(n_gas, -1) for _, F in rays], axis=1))
    path = dict(alt=cat("alt"), dx=cat("dx"), dalt=cat("dalt"))
    return los, path, [G for G, _ in rays]


def dcol_reference(G):
    """The reference d col / d z_t of a ray's long double geometry, [n_gas, n_seg]."""
    return dcol_forward(G["x"], G["nd"], G["vmr"], G["alt"], G["dx"], G["dalt"], LD)


def richardson(zt, h, n_gas=N_GAS_MAX):
    """Richardson-extrapolated central differences of the long double columns of rebuilt geometry, the shells of z_t
    held fixed: (value at step h / 2, |value at h - value at h / 2|: its own error estimate), [n_gas, n_seg] each."""
    z, nd, vmr = case_profiles(n_gas)
    shells = crossed_shells(z, zt)

    def col(at):
        G = geometry_ld(z, nd, vmr, at, shells=shells)
        return columns(G["x"], G["nd"], G["vmr"])

    def central(step):
        step = LD(step)
        return (col(LD(zt) + step) - col(LD(zt) - step)) / (LD(2) * step)

    def extrapolated(step):
        return (LD(4) * central(step / 2) - central(step)) / LD(3)

    r1, r2 = extrapolated(h), extrapolated(h / 2)
    return r2, np.abs(r1 - r2)


def measure_k_plain_dcol(z_tans=Z_TANS, n_gas=N_GAS_MAX):
    """(max, [(z_t, per-gas distances)]) of the plain fp64 derivative against the reference on the case set."""
    rows = []
    for zt in z_tans:
        G, F = ray_case(zt, n_gas)
        plain = dcol_forward(F["x"], F["nd"], F["vmr"], F["alt"], F["dx"], F["dalt"], np.float64)
        rows.append((zt, dist(plain, dcol_reference(G))))
    return float(max(d.max() for _, d in rows)), rows
