"""Line-of-sight geometry for the device LOS pipeline (engine.LimbLOS): limb, slant / nadir and 3-D paths through
spherical shells, and the adaptive LOS stepping of the reference's drivers.

The reference's LineOfSight class (calc_atm_intersections, calc_radtran_steps, calc_SZA_along_los, radtran*) lives in
the absent spect_base_module; what is pinned are its call sites and their knobs:

    los.calc_radtran_steps(planet, lines, max_opt_depth=..., max_T_variation=5., max_Plog_variation=1.)
        spect_main_module.py:2746-2767, 3147; radtran_test_CO.py:184-186; spect_radtran_test.py:175;
        radtran_3Dvs2D_sza30-80_test.py:285-287
    use_tangent_sza / invert_LOS_direction (LOS_order)           spect_main_module.py:2748-2757
    atmosphere on (latitude box, altitude): ['box', 'lin'] temperature, ['box', 'exp'] pressure
        radtran_3Dvs2D_sza30-80_test.py:66-90 (lat_ext = [-90, -75, -60, -30, 30, 60, 75, 90])

so these builders are the build's own definition behind those names: a step is a stretch of the path inside one
altitude shell (and one latitude box); fixed stepping = one step per shell crossing (the benches), adaptive stepping
splits a crossing until the temperature, log-pressure and optical-depth variation of every step stay inside the
bounds.  Everything is vectorised over the segments of a ray (no per-segment Python loops).

Profiles along the path are the ones curgods.f assumes: number density exponential, VMR linear in altitude between
the levels; the column of a segment is curgod_fort_2 over its n_sub + 1 sample points, evaluated on the device.
"""
import numpy as np

TITAN_RADIUS_KM = 2575.0                                   # spect_classes.py:32
LAT_EXT = np.array([-90., -75., -60., -30., 30., 60., 75., 90.])   # radtran_3Dvs2D_sza30-80_test.py:67


def _profiles(z, nd_levels, vmr_levels):
    """Level profiles continued to the top boundary (one more shell of the last thickness) with the last scale height
    / last VMR: (zz, ln nd, vmr) on the len(z) + 1 boundaries."""
    z = np.asarray(z, float)
    nd_levels = np.asarray(nd_levels, float)
    vmr_levels = np.atleast_2d(np.asarray(vmr_levels, float))
    dz = np.diff(z)
    top = z[-1] + (dz[-1] if len(dz) else 10.0)
    lognd = np.log(nd_levels)
    lognd_top = lognd[-1] + (lognd[-1] - lognd[-2]) / dz[-1] * (top - z[-1]) if len(dz) else lognd[-1]
    zz = np.concatenate([z, [top]])
    return z, zz, np.concatenate([lognd, [lognd_top]]), np.concatenate([vmr_levels, vmr_levels[:, -1:]], axis=1)


def _limb_crossings(zz, zt, R):
    """Shell crossings of one limb ray in photon order (far side -> tangent point -> observer): shell index k and the
    path coordinates (km from the tangent point, negative on the far side) of its two ends."""
    return _crossings_at_radius(zz, R + zt, R)


def _crossings_at_radius(zz, rt, R):
    """_limb_crossings of the ray with the tangent RADIUS rt (solar_columns: a ray given by its impact parameter)."""
    lo, hi = R + zz[:-1], R + zz[1:]
    k = np.nonzero(hi > rt)[0]
    s_hi = np.sqrt(hi[k] * hi[k] - rt * rt)
    s_lo = np.where(lo[k] > rt, np.sqrt(np.maximum(lo[k] * lo[k] - rt * rt, 0.0)), 0.0)
    kk = np.concatenate([k[::-1], k])
    a = np.concatenate([-s_hi[::-1], s_lo])
    b = np.concatenate([-s_lo[::-1], s_hi])
    return kk.astype(np.int32), a, b


def limb_path(z, z_tan, R=TITAN_RADIUS_KM):
    """Path segments of a limb ray with tangent height z_tan through spherical shells bounded by the levels z (km), in
    photon order.  Returns (seg_layer[int32], seg_len_km)."""
    z, zz, _, _ = _profiles(z, np.ones(len(z)), np.ones((1, len(z))))
    k, a, b = _limb_crossings(zz, float(z_tan), R)
    return k, b - a


def _sample(a, b, n_sub):
    """n_sub + 1 equally spaced path coordinates per segment, [n_seg, n_sub + 1] (np.linspace per row)."""
    step = (b - a) / n_sub
    s = np.arange(n_sub + 1)[None, :] * step[:, None] + a[:, None]      # np.linspace's own arithmetic
    s[:, -1] = b                                                      # ... which ends exactly on b
    return s


_LOS_GEOMETRY = {}   # (levels, tangent heights, R, n_sub) -> segment / sample-point geometry of limb_los
_LOS_PATH = {}       # the same key -> (dx_dzt, dalt_dzt) of limb_los(path=True)


def _limb_path_derivatives(zz, zt, R, n_sub):
    """(d s_i / d z_t [km / km], d alt_i / d z_t) at the sample points of one limb ray, [n_seg, n_sub + 1] each, the
    crossed shells held fixed.  A shell end at radius hi > r_t lies at s = sqrt(hi^2 - r_t^2) with d s / d z_t = -r_t / s
    (the tangent point: s = 0, derivative 0; far side mirrored), sample point i blends the ends a, b with f = i / n_sub,
    and d alt_i / d z_t = (s_i d s_i + r_t) / (alt_i + R).  With a da = b db = -r_t the numerator is
        -r_t f (1 - f) (b - a)^2 / (a b)            in a shell above the tangent shell,
        r_t (1 - f^2)  /  r_t (1 - (1 - f)^2)       in the tangent shell (near / far side),
    forms without cancellation: exactly 0 on a shell boundary, 1 at the tangent point.  The ends' distances come from
    (hi - r_t)(hi + r_t) with hi - r_t = zz - z_t, which keeps its digits where a level lies just above the ray."""
    rt = R + zt
    k = np.nonzero(R + zz[1:] > rt)[0]
    hi, lo = zz[1:][k], zz[:-1][k]
    s_hi = np.sqrt((hi - zt) * ((R + hi) + rt))
    above = (R + lo) > rt
    s_lo = np.where(above, np.sqrt(np.where(above, (lo - zt) * ((R + lo) + rt), 0.0)), 0.0)
    with np.errstate(divide="ignore"):
        d_hi, d_lo = -rt / s_hi, np.where(above, -rt / np.where(above, s_lo, 1.0), 0.0)
    # photon order: far side (a = -s_hi, b = -s_lo, outermost shell first), then near side (a = s_lo, b = s_hi)
    a = np.concatenate([-s_hi[::-1], s_lo])[:, None]
    b = np.concatenate([-s_lo[::-1], s_hi])[:, None]
    da = np.concatenate([-d_hi[::-1], d_lo])[:, None]
    db = np.concatenate([-d_lo[::-1], d_hi])[:, None]
    i = np.arange(n_sub + 1)[None, :]
    f, g = i / n_sub, (n_sub - i) / n_sub                       # f and 1 - f
    s = a * g + b * f
    ds = da * g + db * f
    tangent = np.concatenate([~above[::-1], ~above])[:, None]
    far = (np.arange(2 * len(k)) < len(k))[:, None]
    # b - a of a shell above the tangent shell from b^2 - a^2 = (hi - lo)(hi + lo): the difference of two long paths
    span = (hi - lo) * ((R + hi) + (R + lo)) / (s_hi + s_lo)
    span = np.concatenate([span[::-1], span])[:, None]
    num_above = -rt * f * g * span * span / np.where(tangent, 1.0, a * b)
    num = np.where(tangent, np.where(far, rt * f * (1.0 + g), rt * g * (1.0 + f)), num_above)
    return ds, num / np.sqrt(s * s + rt * rt)


def limb_los(z, nd_levels, vmr_levels, z_tans, R=TITAN_RADIUS_KM, n_sub=3, path=False):
    """Lines of sight of limb rays through spherical shells (fixed stepping: one step per shell crossing): per ray the
    crossings in photon order, per crossing n_sub + 1 sample points with the number density interpolated exponentially
    and every VMR linearly in altitude between the levels z.  vmr_levels: [n_gas, n_levels].  Returns the LimbLOS
    arguments dict(seg_off, seg_layer, pt_off, x [cm], nd, vmr [n_gas, n_pt]) plus `alt` [n_pt] (km).
    path=True: also `dx_dzt` [n_pt] (cm per km) and `dalt_dzt` [n_pt], the derivatives of x and alt to the ray's own
    tangent altitude with the set of crossed shells held fixed (one-sided where z_t lies on a level: the tangent shell
    is the one above) -- LimbLOS(path=dict(alt=, dx=, dalt=)), the pointing derivative.  No refraction; the other
    builders of this module (3-D, slant / nadir, adaptive stepping) have no such derivative."""
    z, zz, ln, vv = _profiles(z, nd_levels, vmr_levels)
    z_tans = np.atleast_1d(np.asarray(z_tans, float))
    # the geometry depends on the levels and the tangent heights only: a retrieval loop asks for the same rays with
    # new VMR profiles every iteration (it was 11 of the 15 ms of a configs[4] iteration)
    key = (z.tobytes(), z_tans.tobytes(), float(R), int(n_sub))
    geo = _LOS_GEOMETRY.get(key)
    if geo is None:
        seg_off, lay, xs, alts = [0], [], [], []
        for zt in z_tans:
            k, a, b = _limb_crossings(zz, zt, R)
            s = _sample(a, b, n_sub)
            lay.append(k)
            xs.append(s.ravel())
            alts.append((np.sqrt(s * s + (R + zt) ** 2) - R).ravel())
            seg_off.append(seg_off[-1] + len(k))
        n_seg = seg_off[-1]
        geo = (np.array(seg_off, np.int32), np.concatenate(lay).astype(np.int32),
               (np.arange(n_seg + 1) * (n_sub + 1)).astype(np.int32), np.concatenate(xs) * 1e5,
               np.clip(np.concatenate(alts), z[0], zz[-1]))
        if len(_LOS_GEOMETRY) >= 8:
            _LOS_GEOMETRY.pop(next(iter(_LOS_GEOMETRY)))
        _LOS_GEOMETRY[key] = geo
    seg_off, seg_layer, pt_off, x_cm, alts = geo
    nd = np.exp(np.interp(alts, zz, ln))
    vmr = np.array([np.interp(alts, zz, v) for v in vv])
    out = dict(seg_off=seg_off, seg_layer=seg_layer, pt_off=pt_off, x=x_cm, nd=nd, vmr=vmr, alt=alts)
    if path:
        der = _LOS_PATH.get(key)
        if der is None:
            per_ray = [_limb_path_derivatives(zz, zt, float(R), int(n_sub)) for zt in z_tans]
            der = (np.concatenate([d[0].ravel() for d in per_ray]) * 1e5, np.concatenate([d[1].ravel() for d in per_ray]))
            if len(_LOS_PATH) >= 8:
                _LOS_PATH.pop(next(iter(_LOS_PATH)))
            _LOS_PATH[key] = der
        out["dx_dzt"], out["dalt_dzt"] = der
    return out


def sun_in_local_frame(tangent_lat_deg, subsolar_lat_deg, sza_tangent_deg):
    """Unit vector to the sun in the (up, north, east) frame of a tangent point at the given latitude that sees the sun
    at sza_tangent: the hour angle H follows from cos SZA = sin lat sin dec + cos lat cos dec cos H (afternoon side).
    Raises if that SZA does not occur at this latitude."""
    lat, dec, sza = (np.deg2rad(np.asarray(v, float)) for v in (tangent_lat_deg, subsolar_lat_deg, sza_tangent_deg))
    ch = (np.cos(sza) - np.sin(lat) * np.sin(dec)) / (np.cos(lat) * np.cos(dec))
    if np.any(np.abs(ch) > 1.0):
        raise ValueError("a solar zenith angle of %s deg does not occur at latitude %s (subsolar latitude %s)"
                         % (sza_tangent_deg, tangent_lat_deg, subsolar_lat_deg))
    H = np.arccos(ch)
    sun = np.stack([np.cos(dec) * np.cos(H), np.cos(dec) * np.sin(H), np.sin(dec) * np.ones_like(H)], axis=-1)   # x: lon 0, z: pole
    up = np.stack([np.cos(lat), np.zeros_like(lat), np.sin(lat)], axis=-1)
    north = np.stack([-np.sin(lat), np.zeros_like(lat), np.cos(lat)], axis=-1)
    east = np.stack([np.zeros_like(lat), np.ones_like(lat), np.zeros_like(lat)], axis=-1)
    return np.stack([(sun * up).sum(-1), (sun * north).sum(-1), (sun * east).sum(-1)], axis=-1)


def path_state_3d(L, z_tans, sun_local, heading_deg, tangent_lat_deg=0.0, R=TITAN_RADIUS_KM):
    """Per segment of the LOS batch L (limb_los / calc_radtran_steps output): cos SZA and latitude (deg) at the middle
    of the segment, for rays whose tangent points lie at tangent_lat (lon 0), head `heading_deg` east of north there and
    see the sun in the direction sun_local = (up, north, east) components (sun_in_local_frame).  The point at path
    coordinate s is p = r_t up + s d, d = cos(heading) north + sin(heading) east:

        cos SZA(s) = (r_t sun_up + s (sun_north cos h + sun_east sin h)) / |p|,   lat(s) = asin(p_z / |p|)."""
    z_tans = np.atleast_1d(np.asarray(z_tans, float))
    n_rays = len(z_tans)
    sun = np.broadcast_to(np.asarray(sun_local, float), (n_rays, 3))
    hd = np.deg2rad(np.broadcast_to(np.asarray(heading_deg, float), (n_rays,)))
    lat_t = np.deg2rad(np.broadcast_to(np.asarray(tangent_lat_deg, float), (n_rays,)))
    seg_off, pt_off = L["seg_off"], L["pt_off"]
    n_seg = len(L["seg_layer"])
    ray = np.repeat(np.arange(n_rays), np.diff(seg_off))
    s_mid = 0.5 * (L["x"][pt_off[:-1]] + L["x"][pt_off[1:] - 1]) * 1e-5      # km from the tangent point
    rt = R + z_tans[ray]
    norm = np.sqrt(rt * rt + s_mid * s_mid)
    mu = (rt * sun[ray, 0] + s_mid * (sun[ray, 1] * np.cos(hd[ray]) + sun[ray, 2] * np.sin(hd[ray]))) / norm
    pz = rt * np.sin(lat_t[ray]) + s_mid * np.cos(hd[ray]) * np.cos(lat_t[ray])
    lat = np.rad2deg(np.arcsin(np.clip(pz / norm, -1.0, 1.0)))
    assert len(mu) == n_seg
    return mu, lat


def lat_box_index(lat_deg, lat_ext=LAT_EXT):
    """Latitude box of the reference's 3-D atmospheres (['box', ...] interpolation on lat_ext[:-1])."""
    return np.clip(np.searchsorted(np.asarray(lat_ext, float), np.asarray(lat_deg, float), side="right") - 1, 0, len(lat_ext) - 2)


def limb_los_3d(z, nd_levels, vmr_levels, z_tans, sza_tangent_deg, azimuth_deg, R=TITAN_RADIUS_KM, n_sub=3,
                tangent_lat_deg=None, subsolar_lat_deg=None):
    """limb_los for a 3-D atmosphere: every LOS step is its own row of the coefficient tables, because the state along
    the path depends on the local illumination (and latitude), not on altitude alone.  Stands in for the absent sbm
    LineOfSight.calc_atm_intersections + calc_SZA_along_los (spect_main_module.py:2746-2757 with use_tangent_sza =
    False).  Two ways to place the sun:

      tangent_lat_deg None (round 3): azimuth_deg is the angle between the ray and the sun's horizontal direction at
        the tangent point:  cos SZA(s) = (r_t cos SZA_t + s sin SZA_t cos az) / sqrt(r_t^2 + s^2);
      tangent_lat_deg given: the tangent points lie at that latitude, the rays head azimuth_deg east of north and the
        sun stands at subsolar_lat_deg with the hour angle that gives SZA_t there (sun_in_local_frame).

    Returns limb_los's dict with seg_layer = 0 .. n_seg-1 (one coefficient row per step) plus, per step, `seg_alt_layer`
    (the altitude shell), `seg_mu` = cos SZA and `seg_lat` (deg) at the middle of the step."""
    L = limb_los(z, nd_levels, vmr_levels, z_tans, R=R, n_sub=n_sub)
    z_tans = np.atleast_1d(np.asarray(z_tans, float))
    if tangent_lat_deg is None:
        szt = np.deg2rad(np.broadcast_to(np.asarray(sza_tangent_deg, float), z_tans.shape))
        sun = np.stack([np.cos(szt), np.sin(szt), np.zeros_like(szt)], axis=-1)     # sun's horizontal direction = "north"
        lat_t = 0.0
    else:
        lat_t = np.broadcast_to(np.asarray(tangent_lat_deg, float), z_tans.shape)
        sun = sun_in_local_frame(lat_t, 0.0 if subsolar_lat_deg is None else subsolar_lat_deg,
                                 np.broadcast_to(np.asarray(sza_tangent_deg, float), z_tans.shape))
    mu, lat = path_state_3d(L, z_tans, sun, azimuth_deg, lat_t, R=R)
    out = dict(L)
    out["seg_alt_layer"] = L["seg_layer"].copy()
    out["seg_layer"] = np.arange(len(mu), dtype=np.int32)
    out["seg_mu"] = mu
    out["seg_lat"] = lat
    return out


def lat_box_of_segments(L3, lat_limits):
    """The latitude box of every LOS step of a batch that knows its steps' latitudes (`seg_lat`: limb_los_3d, or limb_los
    with path_state_3d's second result put in): 'box' interpolation on the limits of a retrieval set
    (smm.LinearProfile_2D.lats, smm.lat_box): the boxes START at lat_limits, box j holds lat_limits[j] <= lat <
    lat_limits[j + 1], the last one is open-ended; a step south of the first limit takes box 0.  It is lat_box_index on
    the limits closed by +inf.  (smm.lat_box, as the reference, gives a latitude exactly ON the last limit to no box; here
    it belongs to the last one.)  int32 [n_seg]."""
    lim = np.asarray(lat_limits, float)
    return lat_box_index(L3["seg_lat"], np.append(lim, np.inf)).astype(np.int32)


def _alt_bracket(L3, z):
    """Per sample point: the level below (k), and the weights of levels k and k + 1 -- linear in altitude between the
    levels, constant above the last (k + 1 is then the last level again, with weight 0) and below the first."""
    z = np.asarray(z, float)
    alt = np.clip(np.asarray(L3["alt"], float), z[0], z[-1])
    k = np.clip(np.searchsorted(z, alt, side="right") - 1, 0, len(z) - 1)
    k1 = np.minimum(k + 1, len(z) - 1)
    f = np.where(k1 > k, (alt - z[k]) / np.where(k1 > k, z[k1] - z[k], 1.0), 0.0)
    return k, k1, 1.0 - f, f


def _box_of_points(L3, seg_box):
    return np.repeat(np.asarray(seg_box, int), np.diff(np.asarray(L3["pt_off"])))


def box_vmr(L3, z, vmr_boxes, seg_box):
    """VMR [n_pt] at every LOS sample point of a gas whose profile depends on the latitude box: vmr_boxes [n_box, n_lev]
    on the levels z, seg_box [n_seg] the box of every step (lat_box_of_segments).  A sample point takes the profile of its
    STEP's box, linear in altitude between the levels and constant above the last, as _profiles does: sample points are
    listed per step, so a box boundary falls between two steps and the Curtis-Godson column of a step never mixes boxes."""
    v = np.asarray(vmr_boxes, float)
    k, k1, a0, a1 = _alt_bracket(L3, z)
    b = _box_of_points(L3, seg_box)
    return a0 * v[b, k] + a1 * v[b, k1]


def box_profile_weights(L3, z, masks, seg_box):
    """[n_par, n_pt]: the masks of the parameters of a latitude-box profile (masks [n_par, n_box, n_lev]: GridMask2D.mask
    of smm.LinearProfile_2D's parameters) at the LOS sample points, by box_vmr's rule: d vmr(point) / d x_p.  The masks
    times the parameters' values are box_vmr of the set's profile, to rounding."""
    m = np.asarray(masks, float)
    k, k1, a0, a1 = _alt_bracket(L3, z)
    b = _box_of_points(L3, seg_box)
    return a0[None, :] * m[:, b, k] + a1[None, :] * m[:, b, k1]


def slant_los(z, nd_levels, vmr_levels, zenith_deg, R=TITAN_RADIUS_KM, n_sub=3):
    """Upward-looking-from-below / nadir-viewing paths: rays that leave the lowest level z[0] at the given zenith
    angles (0 = nadir view / vertical path) and cross every shell once, in photon order (bottom -> top, the observer
    is above the atmosphere).  The geometry of the reference's planetary (non-limb) cases -- BASELINE configs[0]
    quotes a "40-layer 1D nadir" CO case: a ray of impact parameter b = (R + z[0]) sin(zenith) has the path length
    sqrt(r_hi^2 - b^2) - sqrt(r_lo^2 - b^2) in the shell [r_lo, r_hi].  Same dict as limb_los; combine with
    LimbLOS(initial_temperature=T_surface) for the surface emission behind the path."""
    z, zz, ln, vv = _profiles(z, nd_levels, vmr_levels)
    seg_off, lay, xs, alts = [0], [], [], []
    for zen in np.atleast_1d(np.asarray(zenith_deg, float)):
        if not 0.0 <= zen < 90.0:
            raise ValueError("zenith angle must be in [0, 90)")
        b = (R + z[0]) * np.sin(np.deg2rad(zen))
        lo, hi = R + zz[:-1], R + zz[1:]
        s = _sample(np.sqrt(lo * lo - b * b), np.sqrt(hi * hi - b * b), n_sub)   # path coordinate from the closest approach
        lay.append(np.arange(len(z), dtype=np.int32))
        xs.append(s.ravel())
        alts.append((np.sqrt(s * s + b * b) - R).ravel())
        seg_off.append(seg_off[-1] + len(z))
    alts = np.clip(np.concatenate(alts), z[0], zz[-1])
    nd = np.exp(np.interp(alts, zz, ln))
    vmr = np.array([np.interp(alts, zz, v) for v in vv])
    n_seg = seg_off[-1]
    return dict(seg_off=np.array(seg_off, np.int32), seg_layer=np.concatenate(lay).astype(np.int32),
                pt_off=(np.arange(n_seg + 1) * (n_sub + 1)).astype(np.int32), x=np.concatenate(xs) * 1e5, nd=nd, vmr=vmr, alt=alts)


def calc_radtran_steps(z, temps, press, nd_levels, vmr_levels, z_tans, R=TITAN_RADIUS_KM, n_sub=3, max_T_variation=None,
                       max_Plog_variation=None, max_opt_depth=None, opt_depth_of=None, max_rounds=12):
    """Adaptive LOS stepping with the reference's knobs (radtran_opt: max_T_variation [K], max_Plog_variation [ln P],
    max_opt_depth): every shell crossing of every limb ray is split into equal ALTITUDE slices until, inside each step,
    the temperature (linear in altitude between the levels, ['lin']) varies by at most max_T_variation and ln P
    (['exp']) by at most max_Plog_variation; then steps whose optical depth exceeds max_opt_depth are halved until none
    does (opt_depth_of(steps) -> largest optical depth of every step over the spectral grid; the caller supplies it
    from the coefficient rows on the device, engine.refine_los_by_opt_depth).  None = that bound is off; all three off
    reproduces limb_los's crossings.

    A step carries the state at its own mean altitude: step_temp (linear), step_pres (exponential in altitude) -- its
    coefficient row; `seg_layer` numbers the steps 0 .. n_seg-1 as in limb_los_3d, `seg_alt_layer` is the shell.
    Returns limb_los's dict + seg_alt_layer, step_temp, step_pres, step_alt (mean altitude, km)."""
    z, zz, ln, vv = _profiles(z, nd_levels, vmr_levels)
    temps, press = np.asarray(temps, float), np.asarray(press, float)
    dz_last = zz[-1] - zz[-2]
    # state on the boundaries: T continued constant, ln P with its last scale height
    tt = np.concatenate([temps, temps[-1:]])
    lp = np.log(press)
    lpp = np.concatenate([lp, [lp[-1] + ((lp[-1] - lp[-2]) / (z[-1] - z[-2]) * dz_last if len(z) > 1 else 0.0)]])
    z_tans = np.atleast_1d(np.asarray(z_tans, float))
    rays = []
    for zt in z_tans:
        k, a, b = _limb_crossings(zz, zt, R)
        rt = R + zt
        alt_a, alt_b = np.sqrt(a * a + rt * rt) - R, np.sqrt(b * b + rt * rt) - R
        dT = np.abs(np.interp(alt_b, zz, tt) - np.interp(alt_a, zz, tt))
        dP = np.abs(np.interp(alt_b, zz, lpp) - np.interp(alt_a, zz, lpp))
        n = np.ones(len(k), int)
        if max_T_variation:
            n = np.maximum(n, np.ceil(dT / max_T_variation - 1e-9).astype(int))
        if max_Plog_variation:
            n = np.maximum(n, np.ceil(dP / max_Plog_variation - 1e-9).astype(int))
        # equal altitude slices of each crossing: slice i of n covers alt_a + (alt_b - alt_a) [i, i + 1] / n
        rep = np.repeat(np.arange(len(k)), n)
        i = np.arange(len(rep)) - np.repeat(np.cumsum(n) - n, n)
        f0, f1 = i / n[rep], (i + 1) / n[rep]
        h0 = alt_a[rep] + (alt_b - alt_a)[rep] * f0
        h1 = alt_a[rep] + (alt_b - alt_a)[rep] * f1
        sign = np.where(b[rep] <= 0.0, -1.0, 1.0)               # far side: s < 0
        s0 = sign * np.sqrt(np.maximum((R + h0) ** 2 - rt * rt, 0.0))
        s1 = sign * np.sqrt(np.maximum((R + h1) ** 2 - rt * rt, 0.0))
        # the crossing's own ends exactly (no drift from the altitude round trip)
        first, last = i == 0, i == n[rep] - 1
        s0[first], s1[last] = a[rep][first], b[rep][last]
        rays.append(dict(k=k[rep], a=s0, b=s1, rt=rt))

    def assemble():
        seg_off, lay, xs, alts = [0], [], [], []
        for r in rays:
            s = _sample(r["a"], r["b"], n_sub)
            lay.append(r["k"])
            xs.append(s.ravel())
            alts.append((np.sqrt(s * s + r["rt"] ** 2) - R).ravel())
            seg_off.append(seg_off[-1] + len(r["k"]))
        n_seg = seg_off[-1]
        alt = np.clip(np.concatenate(alts), z[0], zz[-1])
        pt_off = (np.arange(n_seg + 1) * (n_sub + 1)).astype(np.int32)
        mid = np.concatenate([np.sqrt((0.5 * (r["a"] + r["b"])) ** 2 + r["rt"] ** 2) - R for r in rays])
        mid = np.clip(mid, z[0], zz[-1])
        return dict(seg_off=np.array(seg_off, np.int32), seg_layer=np.arange(n_seg, dtype=np.int32),
                    seg_alt_layer=np.concatenate(lay).astype(np.int32), pt_off=pt_off, x=np.concatenate(xs) * 1e5,
                    nd=np.exp(np.interp(alt, zz, ln)), vmr=np.array([np.interp(alt, zz, v) for v in vv]), alt=alt,
                    step_alt=mid, step_temp=np.interp(mid, zz, tt), step_pres=np.exp(np.interp(mid, zz, lpp)))

    L = assemble()
    if max_opt_depth and opt_depth_of is not None:
        for _ in range(max_rounds):
            tau = np.asarray(opt_depth_of(L), float)
            too = tau > max_opt_depth
            if not too.any():
                break
            at = 0
            for r in rays:                                   # halve (in path length) the steps that are too thick
                m = too[at:at + len(r["k"])]
                at += len(r["k"])
                rep = np.repeat(np.arange(len(m)), np.where(m, 2, 1))
                second = np.concatenate([[False], rep[1:] == rep[:-1]])
                mid_s = 0.5 * (r["a"] + r["b"])
                a2 = np.where(second, mid_s[rep], r["a"][rep])
                b2 = np.where(m[rep] & ~second, mid_s[rep], r["b"][rep])
                r["k"], r["a"], r["b"] = r["k"][rep], a2, b2
            L = assemble()
    return L


# ----------------------------------------------------------------------------------------------------------------------
# the sun's ray: slant columns of the single-scattering solar source (engine.solar_source)
# ----------------------------------------------------------------------------------------------------------------------
def _device_columns(L, col_scale):
    """[n_gas, n_seg] Curtis-Godson columns of a LOS dict by the engine's own routine (engine.LimbLOS.columns: on the
    device) -- what a line of sight through the same segments gets."""
    from . import engine
    return engine.LimbLOS(L["seg_off"], L["seg_layer"], L["pt_off"], L["x"], L["nd"], L["vmr"], col_scale=col_scale).columns()


def solar_columns(z, nd_levels, vmr_levels, alt, mu, R=TITAN_RADIUS_KM, n_sub=3, col_scale=None):
    """Slant columns towards the sun: U [n_rows, n_gas, n_layers] (molecules cm^-2 of gas g in the shell above level l)
    along the straight ray from the point at altitude alt[r] (km) that sees the sun at mu[r] = cos SZA, and lit [n_rows].
    The ray has the impact parameter b = (R + alt) sqrt(1 - mu^2); on the limb ray with that tangent radius the point
    sits at the path coordinate s_p = (R + alt) mu and the sun at + infinity, so the sun's ray is that limb ray from
    s_p on (_limb_crossings' own arithmetic, the first crossing cut at s_p):

      mu >= 0   outward through the rest of the point's shell and every shell above;
      mu <  0   down to the tangent radius b and out again: the shells between b and the point are crossed on both
                sides of the tangent point, the part of the point's own shell below it once per crossing;
      mu <  0 and b < R + z[0]   the ray passes below the lowest level: in shadow, lit = False and a row of zeros.

    Every crossing carries n_sub + 1 sample points with limb_los's profiles (_sample, _profiles) and its column is the
    engine's Curtis-Godson column with col_scale -- what a line of sight through the same chord gets; the columns of a
    shell's crossings are added.  No refraction.  A point above the top boundary has an empty, lit row."""
    return _solar_columns(z, nd_levels, vmr_levels, alt, mu, R, n_sub, col_scale, _device_columns)


def _solar_columns(z, nd_levels, vmr_levels, alt, mu, R, n_sub, col_scale, columns):
    """solar_columns with the column routine given: columns(L, col_scale) -> [n_gas, n_seg], L limb_los's dict of the rays'
    crossings (the host tests pass a plain routine, the same on both sides of their comparisons)."""
    z, zz, ln, vv = _profiles(z, nd_levels, vmr_levels)
    n_gas, n_layers = vv.shape[0], len(z)
    lit, L = _solar_rays(z, zz, ln, alt, mu, R, n_sub)
    U = np.zeros((lit.size, n_gas, n_layers))
    if L is None:
        return U, lit
    L["vmr"] = np.array([np.interp(L["alt"], zz, v) for v in vv])
    col = np.asarray(columns(L, col_scale), float)
    row = np.repeat(np.arange(lit.size), np.diff(L["seg_off"]))
    for g in range(n_gas):
        np.add.at(U[:, g, :], (row, L["seg_layer"]), col[g])
    return U, lit


def vertical_columns(z, nd_levels, vmr_levels, R=TITAN_RADIUS_KM, n_sub=3, col_scale=None):
    """Vertical columns of the layers: V [n_gas, n_layers] (molecules cm^-2 of gas g in the shell above level l), what
    engine.diffuse_source takes.  solar_columns for the one point at z[0] with mu = 1: a radial ray's column in a shell
    is that shell's vertical column (the same sampling, profiles and column routine as every other column here)."""
    return _vertical_columns(z, nd_levels, vmr_levels, R, n_sub, col_scale, _device_columns)


def _vertical_columns(z, nd_levels, vmr_levels, R, n_sub, col_scale, columns):
    """vertical_columns with the column routine given, as _solar_columns."""
    z0 = float(np.atleast_1d(np.asarray(z, float))[0])
    U, _ = _solar_columns(z, nd_levels, vmr_levels, [z0], 1.0, R, n_sub, col_scale, columns)
    return np.ascontiguousarray(U[0])


def sza_columns(seg_mu, n_col):
    """The solar zenith angles a 3-D batch's diffuse field is solved at, and each step's weights between them:
    (mu_nodes [n_col], col_w [n_seg, n_col]) for engine.diffuse_source_columns.  The nodes are equally spaced in
    mu = cos SZA from min(seg_mu) to max(seg_mu); a step's weights are linear in mu: at most two non-zeros, adjacent,
    summing to 1, with col_w @ mu_nodes = seg_mu.  With n_col == 1, or steps that span less than 1e-12 in mu, there is one
    node at the mean and every weight is 1."""
    mu = np.asarray(seg_mu, dtype=float).reshape(-1)
    n_col = int(n_col)
    if n_col < 1 or mu.size == 0 or not np.all(np.abs(mu) <= 1.0):
        raise ValueError("sza_columns takes n_col >= 1 and cosines in [-1, 1], one step at the least")
    lo, hi = float(mu.min()), float(mu.max())
    if n_col == 1 or hi - lo < 1e-12:
        return np.array([lo if hi == lo else float(mu.mean())]), np.ones((mu.size, 1))
    nodes = np.linspace(lo, hi, n_col)
    k = np.clip(np.searchsorted(nodes, mu, side="right") - 1, 0, n_col - 2)
    f = np.clip((mu - nodes[k]) / (nodes[k + 1] - nodes[k]), 0.0, 1.0)
    w = np.zeros((mu.size, n_col))
    at = np.arange(mu.size)
    w[at, k], w[at, k + 1] = 1.0 - f, f
    return nodes, w


def _solar_rays(z, zz, ln, alt, mu, R, n_sub):
    """The sun rays of _solar_columns without a profile on them: (lit [n_rows], limb_los's dict of the rays' crossings
    with x, nd and alt but no vmr -- None when no ray crosses anything).  z, zz, ln: _profiles' levels."""
    alt = np.atleast_1d(np.asarray(alt, float))
    mu = np.broadcast_to(np.asarray(mu, float), alt.shape)
    if np.any(np.abs(mu) > 1.0):
        raise ValueError("mu = cos SZA must lie in [-1, 1]")
    n_rows = alt.size
    lit = np.ones(n_rows, bool)
    seg_off, lay, xs, alts = [0], [], [], []
    for r_alt, m in zip(alt, mu):
        rp = R + r_alt
        b = rp * np.sqrt((1.0 - m) * (1.0 + m))
        if m < 0.0 and b < R + z[0]:
            lit[len(seg_off) - 1] = False
            seg_off.append(seg_off[-1])
            continue
        k, a, e = _crossings_at_radius(zz, b, R)
        s_p = rp * m
        keep = e - s_p > 1e-12 * rp      # (a point ON a level: the crossing that ends there, to rounding, is not begun)
        k, a, e = k[keep], np.maximum(a[keep], s_p), e[keep]
        s = _sample(a, e, n_sub)
        lay.append(k)
        xs.append(s.ravel())
        alts.append((np.sqrt(s * s + b * b) - R).ravel())
        seg_off.append(seg_off[-1] + len(k))
    n_seg = seg_off[-1]
    if n_seg == 0:
        return lit, None
    al = np.clip(np.concatenate(alts), z[0], zz[-1])
    return lit, dict(seg_off=np.array(seg_off, np.int32), seg_layer=np.concatenate(lay).astype(np.int32),
                     pt_off=(np.arange(n_seg + 1) * (n_sub + 1)).astype(np.int32), x=np.concatenate(xs) * 1e5,
                     nd=np.exp(np.interp(al, zz, ln)), alt=al)


SOLAR_WEIGHT_BATCH = 8      # masks per column call: what one LOS batch takes as gases


def solar_column_weights(z, nd_levels, masks, par_gas, n_gas, alt, mu, R=TITAN_RADIUS_KM, n_sub=3, col_scale=None):
    """The derivative of solar_columns to column parameters: dU [n_par, n_rows, n_gas, n_layers] = d U / d x_p for
    d vmr_{par_gas[p]}(z_i) / d x_p = masks[p][i] (as LimbScene.profile_weights assumes), and lit [n_rows].  solar_columns
    is linear in the VMR profiles, so this is the same crossings, sampling and column routine with the mask in gas
    par_gas[p]'s place (with that gas's col_scale) and zeros elsewhere; the rays are walked once for all parameters, the
    column routine takes SOLAR_WEIGHT_BATCH masks per call.  Masks may have either sign; a row in shadow is a row of
    zeros.  sum_p x_p dU_p is solar_columns of the profiles sum_p x_p masks_p, to rounding."""
    return _solar_column_weights(z, nd_levels, masks, par_gas, n_gas, alt, mu, R, n_sub, col_scale, _device_columns)


def _solar_column_weights(z, nd_levels, masks, par_gas, n_gas, alt, mu, R, n_sub, col_scale, columns):
    """solar_column_weights with the column routine given, as _solar_columns."""
    masks = np.atleast_2d(np.asarray(masks, float))
    par_gas = np.atleast_1d(np.asarray(par_gas, int))
    n_par, n_gas = masks.shape[0], int(n_gas)
    if par_gas.shape != (n_par,) or (n_par and (par_gas.min() < 0 or par_gas.max() >= n_gas)):
        raise ValueError("par_gas must name a gas 0 .. n_gas - 1 for every mask")
    if masks.shape[1] != len(np.atleast_1d(z)):
        raise ValueError("the masks must be on the levels z")
    z, zz, ln, mm = _profiles(z, nd_levels, masks)
    lit, L = _solar_rays(z, zz, ln, alt, mu, R, n_sub)
    dU = np.zeros((n_par, lit.size, n_gas, len(z)))
    if L is None or n_par == 0:
        return dU, lit
    scale = np.ones(n_gas) if col_scale is None else np.asarray(col_scale, float)
    row = np.repeat(np.arange(lit.size), np.diff(L["seg_off"]))
    for p0 in range(0, n_par, SOLAR_WEIGHT_BATCH):
        ps = range(p0, min(p0 + SOLAR_WEIGHT_BATCH, n_par))
        Lb = dict(L, vmr=np.array([np.interp(L["alt"], zz, mm[p]) for p in ps]))
        col = np.asarray(columns(Lb, [scale[par_gas[p]] for p in ps]), float)
        for i, p in enumerate(ps):
            np.add.at(dU[p, :, par_gas[p], :], (row, L["seg_layer"]), col[i])
    return dU, lit


def vertical_column_weights(z, nd_levels, masks, par_gas, n_gas, R=TITAN_RADIUS_KM, n_sub=3, col_scale=None):
    """The derivative of vertical_columns to column parameters: dV [n_par, n_gas, n_layers] = d V / d x_p, what
    engine.diffuse_jacobian takes.  solar_column_weights for the one point at z[0] with mu = 1, as vertical_columns is to
    solar_columns; sum_p x_p dV_p is vertical_columns of the profiles sum_p x_p masks_p, to rounding."""
    return _vertical_column_weights(z, nd_levels, masks, par_gas, n_gas, R, n_sub, col_scale, _device_columns)


def _vertical_column_weights(z, nd_levels, masks, par_gas, n_gas, R, n_sub, col_scale, columns):
    """vertical_column_weights with the column routine given, as _solar_columns."""
    z0 = float(np.atleast_1d(np.asarray(z, float))[0])
    dU, _ = _solar_column_weights(z, nd_levels, masks, par_gas, n_gas, [z0], 1.0, R, n_sub, col_scale, columns)
    return np.ascontiguousarray(dU[:, 0])


def hg_phase(cos_theta, g):
    """Henyey-Greenstein phase function P(Theta) = (1 - g^2) / (1 + g^2 - 2 g cos Theta)^(3/2), normalised so that its
    mean over the sphere is 1 (int P dOmega = 4 pi); g: the asymmetry parameter, |g| < 1."""
    g = float(g)
    if not abs(g) < 1.0:
        raise ValueError("the asymmetry parameter must lie in (-1, 1)")
    c = np.asarray(cos_theta, float)
    return (1.0 - g * g) / (1.0 + g * g - 2.0 * g * c) ** 1.5


def hg_phase_dg(cos_theta, g):
    """d hg_phase / d g, analytic: with D = 1 + g^2 - 2 g cos Theta, -(2 g D + 3 (1 - g^2)(g - cos Theta)) / D^(5/2) -- what
    the order-one rows need for a direction in the asymmetry parameter; its mean over the sphere is 0."""
    g = float(g)
    if not abs(g) < 1.0:
        raise ValueError("the asymmetry parameter must lie in (-1, 1)")
    c = np.asarray(cos_theta, float)
    D = 1.0 + g * g - 2.0 * g * c
    return -(2.0 * g * D + 3.0 * (1.0 - g * g) * (g - c)) / D ** 2.5


def solar_irradiance(grid, t_sun=5772.0, r_sun_km=695700.0, dist_km=9.58 * 1.495978707e8):
    """The irradiance of a black-body sun on the grid (cm^-1) at the planet: pi B(nu, t_sun) (r_sun / dist)^2, with the
    Planck function of the limb calls' initial intensity, B = 2 h c^2 nu^3 / (exp(c2 nu / T) - 1) in erg s^-1 cm^-2 sr^-1
    (cm^-1)^-1 -- the units of the emission rows; the result is per unit area, erg s^-1 cm^-2 (cm^-1)^-1.  Defaults: the
    sun seen from Saturn's mean distance."""
    h, c, k = 6.62607015e-34 * 1.e7, 299792458.0 * 1.e2, 1.380649e-23 * 1.e7      # sr_constants.hpp
    nu = np.asarray(grid, float)
    B = 2 * h * (c * c) * (nu * nu * nu) / (np.exp((h * c / k) * nu / float(t_sun)) - 1)
    return np.pi * B * (float(r_sun_km) / float(dist_km)) ** 2
