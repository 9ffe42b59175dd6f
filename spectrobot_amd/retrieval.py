"""Forward model + retrieval loop around the hot path: the structure of the reference's
`inversion_fast_limb` / `radtrans` (spect_main_module.py:2598-2987, 2990-3287) on the GPU engine.

The reference's loop is, per iteration: LOS stepping and coefficients per LOS (`calc_radtran_steps`),
radiances + derivatives per spectral split (`radtran_fast`), `hires_to_lowres`, `FOV_integr_1D` over the
three LOS of every pixel, `chicalc`, the stopping rule (|dchi2|/chi2 < chi_threshold, or chi2 raised),
`inversion_algebra`, `add_clim(profile)`.  Planet / atmosphere / LineOfSight / VIMSPixel are classes of the
absent spect_base_module; `LimbScene` is the minimal stand-in the loop needs (a 1-D atmosphere on altitude
levels, gases with VMR profiles, limb pixels with three lines of sight each).  What runs where:

  per scene      engine.LineSet per gas (lines -> HBM once)
  per iteration  coefficients of every gas whose temperature / vibrational temperatures changed (once if
                 only VMRs are retrieved, as in the reference's drivers: radtran_3D_ch4.py:127-170),
                 engine.limb_rays_jacobian: columns on the device, radiances and d rad / d x_p for ALL LOS
                 of ALL pixels in one launch, engine.hires_to_lowres for radiances and derivatives
  host           FOV integration, chi square, the n_par x n_par algebra (smm mirror), bookkeeping
"""
import numpy as np

from . import engine
from . import geometry
from . import spect_main_module as smm
from . import synthetic as syn


STEP_IN_ONE_CALL = True   # inversion_fast_limb: forward model + chi square + the optimal-estimation algebra of an iteration
                          # in one library call (engine.retrieval_step); False: the algebra in numpy (the check)
LOOP_IN_ONE_CALL = True   # ... and the loop around it too (engine.retrieval_loop) when the coefficient spectra stay fixed; False: the
                          # loop below, an engine.retrieval_step per iteration (the check)
ONE_CALL = True   # simulate(arrays=True): the iteration's forward model in one library call (engine.retrieval_forward);
                  # False: columns + Jacobians, instrument step and FOV as separate calls (the A/B partner and the check)


class Spectrum(object):
    """Low-resolution spectrum holder with the attributes the smm algebra reads (.spectrum, .spectral_grid)."""

    def __init__(self, spectrum, grid=None):
        self.spectrum = np.asarray(spectrum, dtype=float)
        self.spectral_grid = None if grid is None else _Grid(grid)


class _Grid(object):
    def __init__(self, g):
        self.grid = np.asarray(g, dtype=float)


class Gas(object):
    """One absorber: its line set on the scene's grid, isotopic abundance, VMR profile on the altitude levels
    and (non-LTE) vibrational temperatures [n_levels, n_layers].
    self_broadening: the line set carries self-broadening coefficients (engine.LineSet.set_line_shape) and the scene
    hands it the gas's own partial pressure, vmr x press of the layers, before every coefficient build.  The VMR
    Jacobians hold the coefficients fixed -- the dependence of the Lorentz width on the gas's own VMR is not
    differentiated; a retrieval refreshes the coefficients between its iterations (coefficients(refresh=True)).
    Every Gas -- an isotopologue with its own iso_ratio too -- takes one of the scene's gas slots: eight in inversion_state,
    inversion_boxes, simulate_boxes and simulate(bayes_set=None), four in the other drivers (see TableGas)."""

    def __init__(self, name, lineset, vmr, iso_ratio=1.0, tvib=None, self_broadening=False):
        self.name, self.lineset, self.iso_ratio = name, lineset, float(iso_ratio)
        self.vmr = np.asarray(vmr, dtype=float)
        self.tvib = tvib
        self.self_broadening = bool(self_broadening)
        self.coeffs = None      # (abs, emi) CUDA [n_layers, n_grid], computed on demand

    def set_self_pressure(self, press):
        """The line set's self pressure for the coefficient build that follows: vmr x press (hPa) when self_broadening."""
        if self.self_broadening:
            self.lineset.set_self_pressure(self.vmr * np.asarray(press, dtype=float))

    def add_clim(self, profile):
        """New VMR profile (planet.gases[gas].add_clim, spect_main_module.py:2625, 2985)."""
        self.vmr = np.asarray(profile, dtype=float)


class LevelGas(Gas):
    """A non-LTE gas on the level-factored route, for retrievals of its vibrational temperatures: it owns an
    engine.LevelFactored on the scene's (T, P) rows -- the pair tables, built once per scene (and spectral shard) -- and
    a reference tvib0 [n_levels, n_layers]; its coefficients are lf.steps(rows, tvib), recombined only when tvib was
    changed (set_tvib): a combine of the resident tables, never a walk of the lines."""

    def __init__(self, name, lineset, vmr, tvib0, iso_ratio=1.0, dT=None, self_broadening=False):
        """dT: handed to engine.LevelFactored -- the tables also at T + dT, for the temperature derivative of the
        coefficients (layer_coefficients(derivative=True): a retrieval with a TempProfile needs it)."""
        tvib0 = np.array(tvib0, dtype=float)
        if tvib0.ndim != 2 or tvib0.shape[0] != max(int(np.size(lineset.level_energies)), 1):
            raise ValueError("tvib0 must be [n_levels, n_layers] for the line set's levels")
        Gas.__init__(self, name, lineset, vmr, iso_ratio=iso_ratio, tvib=tvib0.copy(), self_broadening=self_broadening)
        self.tvib0, self.dT = tvib0, dT
        self.lf, self._lf_key, self._combined, self.dcoeffs = None, None, None, None

    @property
    def n_levels(self):
        return self.tvib0.shape[0]

    def set_tvib(self, tvib):
        tvib = np.array(tvib, dtype=float)
        if tvib.shape != self.tvib0.shape:
            raise ValueError("tvib must be [n_levels, n_layers] like tvib0")
        self.tvib = tvib

    def layer_coefficients(self, temps, press, g_lo=0, g_hi=None, derivative=False):
        """(abs, emi) on the layer stack from the pair tables (LimbScene.coefficients calls this).  New temperatures or
        pressures on the same number of rows and the same shard rebuild the tables in place (LevelFactored.rebuild).
        derivative=True also leaves (d abs / dT, d emi / dT) in self.dcoeffs (LevelFactored.steps(derivative=True))."""
        self.set_self_pressure(press)
        key = (np.asarray(temps, float).tobytes() + (self.vmr.tobytes() if self.self_broadening else b""),
               np.asarray(press, float).tobytes(), int(g_lo), g_hi)
        if self.lf is None or self._lf_key[2:] != key[2:] or self.lf.temps.size != len(temps) or self.lf.dT != self.dT:
            self.lf = engine.LevelFactored(self.lineset, temps, press, dT=self.dT, g_lo=g_lo, g_hi=g_hi)
            self._lf_key, self._combined = key, None
        elif self._lf_key != key:
            self.lf.rebuild(temps, press)
            self._lf_key, self._combined = key, None
        self.rows = np.arange(len(temps), dtype=np.int32)
        tv = np.asarray(self.tvib, float).tobytes()
        if self._combined != tv or self.coeffs is None or (derivative and self.dcoeffs is None):
            if derivative:
                self.coeffs, self.dcoeffs = self.lf.steps(self.rows, tvib=self.tvib, derivative=True)
            else:
                self.coeffs, self.dcoeffs = self.lf.steps(self.rows, tvib=self.tvib), None
            self._combined = tv
        return self.coeffs


class TableGas(Gas):
    """An absorber without lines: an engine.AbsorberTable (cross-section, CIA or extinction table) as a gas of the scene.
    Its pair is abs = scale x table(nu, T[, P]) per unit of whatever the VMR counts, emi = abs B(nu, T) (source=False: no
    emission), and the existing columns apply: a cross-section table (cm^2 per molecule) needs no scale; a CIA pair
    (cm^5 per molecule^2) takes the partner's number density, scale=lambda scene: scene.nd * x_partner, so that abs is
    cm^2 per molecule of the gas that carries the VMR; a haze is a TableGas whose "VMR" is extinction per unit density.
    scale: None, an array per layer, or a callable (scene) -> array; held fixed under d / dT (as TempProfile holds columns
    and pressure fixed).  A retrieval set named after the gas is an ordinary column set.

    A TableGas takes one of the scene's gas slots: eight in inversion_state, inversion_boxes, simulate_boxes and
    simulate(bayes_set=None) (engine.max_gases()), four in simulate with a bayes_set, inversion_fast_limb, inversion and
    radtrans, whose kernels keep four gas slots (engine.max_gases(folded=True)).  accumulate_into=<name of a plain Gas>: the table is
    folded into that line gas's pair instead -- added to its (abs, emi) and, in a temperature retrieval, to its analytic
    row derivatives -- sharing that gas's VMR and iso_ratio; it then has no slot, no VMR and no retrieval set of its
    own (its vmr and iso_ratio arguments are ignored).

    solar=dict(albedo=, g=): the gas scatters sunlight once into the line of sight (single-scattering albedo, Henyey-
    Greenstein asymmetry parameter).  In a LimbScene with a sun its emission rows are thermal + solar: the scene adds
    sca S to a copy of the thermal pair's emi (engine.solar_source; `thermal` keeps the cached pair).  The solar
    attenuation is held fixed under every Jacobian within one linearisation.  Under a Sun(multiple=True) the rows also
    carry the diffuse field's light (orders two and above, engine.diffuse_source), with `albedo` as the single-scattering
    albedo and `g` as the asymmetry parameter of a delta-scaled two-stream solve; g must then be >= -0.5."""

    def __init__(self, name, table, vmr, scale=None, source=True, iso_ratio=1.0, accumulate_into=None, solar=None):
        Gas.__init__(self, name, None, vmr, iso_ratio=iso_ratio)
        self.table, self.scale, self.source, self.accumulate_into = table, scale, bool(source), accumulate_into
        self.dcoeffs, self._key = None, None
        self.solar, self.thermal = None, None
        if solar is not None:
            if accumulate_into is not None:
                raise ValueError("TableGas %r: solar= needs a gas slot of its own (the scatterer's absorption rows are the "
                                 "source's sca), accumulate_into=%r gives it none" % (name, accumulate_into))
            if set(solar) != {"albedo", "g"} or not 0.0 <= float(solar["albedo"]) <= 1.0 or not abs(float(solar["g"])) < 1.0:
                raise ValueError("solar=dict(albedo=<0 .. 1>, g=<asymmetry parameter, |g| < 1>)")
            self.solar = dict(albedo=float(solar["albedo"]), g=float(solar["g"]))

    def scale_of(self, scene):
        """The scale per layer as an array, or None."""
        sc = self.scale(scene) if callable(self.scale) else self.scale
        if sc is None:
            return None
        sc = np.ascontiguousarray(np.broadcast_to(np.asarray(sc, dtype=float), scene.temps.shape))
        return sc

    def cache_key(self, scene, g_lo, g_hi):
        """What the pair depends on, by content: temperatures, pressures, scale, shard (and the source switch)."""
        sc = self.scale_of(scene)
        return (scene.temps.tobytes(), scene.press.tobytes(), None if sc is None else sc.tobytes(), int(g_lo), int(g_hi),
                self.source)

    def layer_coefficients(self, scene, g_lo=0, g_hi=None, derivative=False):
        """(abs, emi) on the scene's layers over [g_lo, g_hi), recomputed when cache_key moved; derivative=True also leaves
        the ANALYTIC (d abs / dT, d emi / dT) in self.dcoeffs -- the same launch, no second build."""
        g_hi = len(scene.grid) if g_hi is None else int(g_hi)
        key = self.cache_key(scene, g_lo, g_hi)
        if self._key != key or self.coeffs is None or (derivative and self.dcoeffs is None):
            res = self.table.layers(scene.temps, scene.grid, press=scene.press, scale=self.scale_of(scene), source=self.source,
                                    derivative=derivative, g_lo=g_lo, g_hi=g_hi)
            self.coeffs, self.dcoeffs = res if derivative else (res, None)
            self._key, self.coeffs_shard = key, (g_lo, g_hi)
            self.thermal = self.coeffs      # (a solar gas: the scene puts (abs, thermal emi + solar rows) into coeffs)
        return self.coeffs


class Sun(object):
    """The sun of a LimbScene: solar zenith angle at the tangent point and phase angle (sun - target - observer), in
    degrees, and the irradiance at the planet on the scene's grid [n_grid] (geometry.solar_irradiance), in units
    consistent with the scene's emission rows.  The scattering angle is 180 deg - phase.

    multiple=True: the solar gases' emission rows also carry sunlight scattered twice or more -- the diffuse field of a
    plane-parallel two-stream solve under the (spherical, delta-scaled) direct beam, engine.diffuse_source, DESIGN.md
    4.11b; order one stays the single-scattering rows.  surface_albedo (0 .. 1) is the Lambertian albedo of what lies
    BELOW z[0]: a scene whose grid starts above the ground uses 0, so that everything below absorbs.  It is read with
    multiple=True only.  By default the diffuse rows are held fixed under every Jacobian within one linearisation, as the
    other solar rows are; their derivative to VMR parameters is LimbScene.diffuse_jacobian
    (inversion_state(diffuse_jacobian=True)); to T and Tvib it is not built."""

    def __init__(self, sza_deg, phase_deg, irradiance, multiple=False, surface_albedo=0.0):
        self.sza_deg, self.phase_deg = float(sza_deg), float(phase_deg)
        self.irradiance = np.ascontiguousarray(irradiance, dtype=float)
        if self.irradiance.ndim != 1 or not np.all(np.isfinite(self.irradiance)) or np.any(self.irradiance < 0):
            raise ValueError("the irradiance is a finite, non-negative array on the scene's grid")
        self.multiple, self.surface_albedo = bool(multiple), float(surface_albedo)
        if not 0.0 <= self.surface_albedo <= 1.0:
            raise ValueError("surface_albedo is a Lambertian albedo in [0, 1]")

    @property
    def mu(self):
        return float(np.cos(np.deg2rad(self.sza_deg)))

    @property
    def cos_scattering(self):
        return float(np.cos(np.deg2rad(180.0 - self.phase_deg)))

    def key(self):
        key = (self.sza_deg, self.phase_deg, engine._content_key(self.irradiance))
        return key + (True, self.surface_albedo) if self.multiple else key


class ThermalScattering(object):
    """Thermal emission as a source of the diffuse field of a LimbScene (engine.diffuse_thermal_source):
    with it every TableGas(solar=...) of the scene is a thermal scatterer -- `albedo` its single-scattering albedo, `g` its
    asymmetry parameter, g >= -0.5 -- with or without a Sun.  Such a gas's emission rows are then its own emission by
    Kirchhoff's law, (1 - albedo) abs B, and the diffuse field of the layers' thermal emission (and, under a
    Sun(multiple=True), of the sunlight, in the same solve) scattered into the line of sight; order one of the sunlight
    stays the single-scattering rows.  Without it such a gas emits abs B, as if all of its extinction were absorption.
    surface_temperature [K]: a Lambertian surface of emissivity 1 - surface_albedo BELOW z[0] emits at it (None: nothing
    below emits).  surface_albedo (0 .. 1) is the albedo of that surface; a Sun(multiple=True) of the same scene must
    carry the same value.  The rows are held fixed under every Jacobian within one linearisation; their derivatives are
    not built: a scene with it refuses diffuse_jacobian=True, a HazeOptics set and a TempProfile set.  The 3-D route,
    LimbScene.sunlit_steps, does not look at it: its rows stay thermal abs B + the sun's."""

    def __init__(self, surface_temperature=None, surface_albedo=0.0):
        self.surface_temperature = None if surface_temperature is None else float(surface_temperature)
        self.surface_albedo = float(surface_albedo)
        if self.surface_temperature is not None and not (np.isfinite(self.surface_temperature) and self.surface_temperature > 0.0):
            raise ValueError("surface_temperature is a temperature in K (> 0), or None for no emitting surface")
        if not 0.0 <= self.surface_albedo <= 1.0:
            raise ValueError("surface_albedo is a Lambertian albedo in [0, 1]")

    def key(self):
        return (self.surface_temperature, self.surface_albedo)


def _refuse_thermal_scattering(scene, what):
    if getattr(scene, "thermal_scattering", None) is not None:
        raise ValueError("%s on a scene with thermal_scattering: the tangent kernels do not know the thermal source of the "
                         "diffuse field (its rows are held fixed within a linearisation, their derivatives are not built)" % what)


def _refuse_many_slots(scene, who):
    """The drivers whose kernels keep four gas slots refuse a larger scene before any device call."""
    limit = engine.max_gases(folded=True)
    if len(scene.gases) > limit:
        raise ValueError("%s: a scene of %d gas slots, the call takes at most max_gases(folded=True) = %d (inversion_state, "
                         "inversion_boxes, simulate_boxes and simulate(bayes_set=None) take %d; TableGas(accumulate_into=...) "
                         "takes no slot)" % (who, len(scene.gases), limit, engine.max_gases()))


def _refuse_table_gas(g, who):
    if isinstance(g, TableGas):
        raise ValueError("%s works on line lists: gas %r is a TableGas (a tabulated absorber has no lines and no levels)" % (who, g.name))


class TvibProfile(smm.LinearProfile_1D_new):
    """The retrieval set of one level's vibrational temperatures: named "tvib:<gas>:<level>", its parameters the nodes
    of an OFFSET profile (K) that is added to the gas's reference, Tvib_L = tvib0[L] + sum_p mask_p x_p, the masks
    those of alt_triangle on the scene's altitude levels (engine.level_node_weights).  An offset may have either sign:
    no parameter is constrained positive."""

    def __init__(self, gas, level, alt_grid, alt_nodes, apriori_err, apriori=None, first_guess=None):
        n = len(list(alt_nodes))
        smm.LinearProfile_1D_new.__init__(self, "tvib:%s:%d" % (gas, int(level)), alt_grid, alt_nodes,
                                          np.zeros(n) if apriori is None else apriori, apriori_err, first_guess_prof=first_guess)
        self.gas, self.level = gas, int(level)
        for par in self.set:
            par.constrain_positive = False


class TempProfile(smm.LinearProfile_1D_new):
    """The retrieval set of the kinetic temperature: named "temp", its parameters the nodes of an OFFSET profile (K) that
    is added to the scene's reference temperatures, T = temps0 + sum_p mask_p x_p, the masks those of alt_triangle on the
    scene's altitude levels (engine.level_node_weights).  No parameter is constrained positive.  The Jacobian holds
    pressure, columns and vibrational temperatures fixed (engine.temperature_jacobian's definition): the number densities
    and the LOS columns do not follow the offset.  Their part of a temperature change is a set of ordinary column
    parameters, which a caller who wants it adds as VMR sets."""

    def __init__(self, alt_grid, alt_nodes, apriori_err, apriori=None, first_guess=None):
        n = len(list(alt_nodes))
        smm.LinearProfile_1D_new.__init__(self, "temp", alt_grid, alt_nodes, np.zeros(n) if apriori is None else apriori,
                                          apriori_err, first_guess_prof=first_guess)
        for par in self.set:
            par.constrain_positive = False


INSTR_SET = "instr"    # the name of the retrieval set of the instrument's band calibration (BandCalibration)


class BandCalibration(smm.RetSet):
    """The retrieval set of the instrument's band calibration, named "instr": up to three scalar parameters,
        shift     (nm)  every band centre moves by it
        slope     (-)   the shift per nm of distance from the mean band centre
        ln_width  (-)   the logarithm of a common factor on the ILS widths
    so that bands_nm = bands_nm0 + shift + slope (bands_nm0 - mean(bands_nm0)) and widths_nm = widths_nm0 exp(ln_width).
    Each is switched on by giving it (apriori, apriori_err) or (apriori, apriori_err, first_guess); a parameter left None
    is not retrieved and stands at 0.  No parameter is constrained positive.  The Jacobian columns come from the two
    instrument rows of the band integrals (engine.hires_to_lowres_instrument: d / d centre, d / d ln width, the windows'
    membership held fixed) by the chain rule, jacobian_rows."""
    KEYS = ("shift", "slope", "ln_width")

    def __init__(self, shift=None, slope=None, ln_width=None):
        self.name, self.set = INSTR_SET, []
        mask = smm.GridMask([0.0], [1.0], 'box')    # (a scalar: nothing to mask)
        for key, spec in zip(self.KEYS, (shift, slope, ln_width)):
            if spec is None:
                continue
            spec = tuple(float(v) for v in spec)
            if len(spec) not in (2, 3):
                raise ValueError("%s must be (apriori, apriori_err) or (apriori, apriori_err, first_guess)" % key)
            self.set.append(smm.RetParam(INSTR_SET, key, mask, spec[0], spec[1], first_guess=spec[2] if len(spec) == 3 else None,
                                         constrain_positive=False))
        if not self.set:
            raise ValueError("a BandCalibration with no parameter switched on")
        self.n_par = len(self.set)

    def value(self, key):
        """The current value of shift / slope / ln_width; 0 for one that is switched off."""
        return float(sum(p.value for p in self.set if p.key == key))

    def bands(self, bands_nm0, widths_nm0):
        """(bands_nm, widths_nm) of the current parameters from the nominal ones."""
        b0, w0 = np.asarray(bands_nm0, float), np.asarray(widths_nm0, float)
        return b0 + self.value("shift") + self.value("slope") * (b0 - b0.mean()), w0 * np.exp(self.value("ln_width"))

    def jacobian_rows(self, bands_nm0, d_centre, d_lnwidth):
        """The derivatives of band values [..., n_bands] to the set's parameters, [..., n_par, n_bands] in the set's order,
        from their derivatives to the band centres (per nm) and to the logarithm of the widths: the chain rule of bands()."""
        b0 = np.asarray(bands_nm0, float)
        rows = dict(shift=d_centre, slope=d_centre * (b0 - b0.mean()), ln_width=d_lnwidth)
        return np.stack([np.asarray(rows[p.key], float) for p in self.set], axis=-2)


POINTING_SET = "pointing"    # the name of the retrieval set of the pointing offset (Pointing)


class Pointing(smm.RetSet):
    """The retrieval set of the pointing, named "pointing": one scalar `offset` [km] common to all pixels, added to every
    line of sight's tangent altitude (LimbPixel.los_alts() + offset).  Given as (apriori, apriori_err) or (apriori,
    apriori_err, first_guess); not constrained positive.  Its Jacobian column is the pointing row of the mixed-state calls
    (engine.limb_rays_state_jacobian / limb_rays_state_bands with pointing=True): d / d z_t of every ray's own tangent
    altitude with the crossed shells held fixed, through the field of view like any other row.  Limb rays of
    geometry.limb_los in a 1-D scene only: 3-D paths, slant / nadir paths, adaptive stepping, observer order, the
    resident-handle routes and refraction have no such row; per-pixel offsets are not part of this set.  Retrieved by
    inversion_state; the other drivers refuse the set."""

    def __init__(self, offset):
        spec = tuple(float(v) for v in offset)
        if len(spec) not in (2, 3):
            raise ValueError("offset must be (apriori, apriori_err) or (apriori, apriori_err, first_guess)")
        mask = smm.GridMask([0.0], [1.0], 'box')    # (a scalar: nothing to mask)
        self.name = POINTING_SET
        self.set = [smm.RetParam(POINTING_SET, "offset", mask, spec[0], spec[1], first_guess=spec[2] if len(spec) == 3 else None,
                                 constrain_positive=False)]
        self.n_par = 1

    def offset(self):
        """The current offset [km]."""
        return float(self.set[0].value)


OPTICS_SET = "optics"


class HazeOptics(smm.RetSet):
    """The retrieval set of a sunlit haze's optics, named "optics": scalar parameters only -- the single-scattering albedo
    and the asymmetry parameter of solar gases (TableGas(solar=dict(albedo=, g=))) and the surface albedo of a
    Sun(multiple=True).  albedo={gas: spec}, g={gas: spec}, surface_albedo=spec, each spec (apriori, apriori_err) or
    (apriori, apriori_err, first_guess); none is constrained positive by the algebra.  After every update the values are
    projected into the library's domain (project(), called where the state goes into the scene): albedo into the CLOSED
    interval [0, 1], surface_albedo into the CLOSED [0, 1], g into [-0.5, 1) -- closed at -0.5, OPEN at 1, where the
    projection stops at 1 - 2^-20.  The Jacobian columns are LimbScene.optics_jacobian's, the full derivative of the
    radiances at the current state.  In thin single scattering ssa x extinction is one number: a state with both a
    haze's profile and its albedo is degenerate.  Retrieved by inversion_state; the other drivers refuse the set."""
    G_MAX = 1.0 - 2.0 ** -20

    def __init__(self, albedo=None, g=None, surface_albedo=None):
        mask = smm.GridMask([0.0], [1.0], 'box')    # (scalars: nothing to mask)
        self.name, self.set, self.keys = OPTICS_SET, [], []
        specs = [(("albedo", gas), s) for gas, s in (albedo or {}).items()] + [(("g", gas), s) for gas, s in (g or {}).items()]
        if surface_albedo is not None:
            specs.append((("surface_albedo", None), surface_albedo))
        if not specs:
            raise ValueError("HazeOptics needs at least one of albedo={gas: spec}, g={gas: spec}, surface_albedo=spec")
        for key, spec in specs:
            spec = tuple(float(v) for v in spec)
            if len(spec) not in (2, 3):
                raise ValueError("a spec is (apriori, apriori_err) or (apriori, apriori_err, first_guess)")
            lo, hi = self.domain(key[0])
            if not (lo <= spec[0] <= hi and lo <= spec[-1] <= hi) or not spec[1] > 0.0:
                raise ValueError("%s: a priori and first guess lie in [%g, %g], the error is positive" % (key[0], lo, hi))
            label = key[0] if key[1] is None else "%s:%s" % key
            self.set.append(smm.RetParam(OPTICS_SET, label, mask, spec[0], spec[1], first_guess=spec[2] if len(spec) == 3 else None,
                                         constrain_positive=False))
            self.keys.append(key)
        self.n_par = len(self.set)

    @classmethod
    def domain(cls, kind):
        return (-0.5, cls.G_MAX) if kind == "g" else (0.0, 1.0)

    def project(self):
        """The values into the library's domain (the class docstring says which ends are closed)."""
        for key, par in zip(self.keys, self.set):
            lo, hi = self.domain(key[0])
            par.value = float(min(max(float(par.value), lo), hi))

    def values(self):
        return [float(par.value) for par in self.set]


def _refuse_instr(bayes_set, who):
    sets = getattr(bayes_set, "sets", {}) if bayes_set is not None else {}
    if OPTICS_SET in sets:
        raise ValueError("%s does not take the retrieval set %r (HazeOptics): use inversion_state" % (who, OPTICS_SET))
    if INSTR_SET in sets:
        raise ValueError("%s does not take the retrieval set %r (BandCalibration): use inversion_state" % (who, INSTR_SET))
    if POINTING_SET in sets:
        raise ValueError("%s does not take the retrieval set %r (Pointing): use inversion_state" % (who, POINTING_SET))


class StateWeights(object):
    """LimbScene.state_weights' result: the column block (par_gas [n_col], par_w_col [n_col, n_pt]), the level block
    (level_gas: the LevelGas or None, gas: its index, par_level [n_lev], par_w_lev [n_lev, n_layers]), the row block
    (par_w_temp [n_row, n_layers]: the temperature nodes' masks; None: no such parameter) and perm [n_par]: the row of the
    call's Jacobian (column parameters, then level parameters, then row parameters) that belongs to BayesSet parameter i.
    level_gases: every LevelGas with a Tvib set, in the order the BayesSet first names them (state_weights with
    several_level_gases: any number; otherwise [level_gas] or []), gases: their indices in the scene, par_lgas [n_lev]: the
    entry of level_gases a level parameter belongs to."""

    def __init__(self, par_gas, par_w_col, level_gas, gas, par_level, par_w_lev, perm, par_w_temp=None, level_gases=None,
                 gases=None, par_lgas=None):
        self.par_gas, self.par_w_col, self.level_gas, self.gas = par_gas, par_w_col, level_gas, gas
        self.par_level, self.par_w_lev, self.perm = par_level, par_w_lev, perm
        self.par_w_temp = np.zeros((0, np.shape(par_w_lev)[1])) if par_w_temp is None else par_w_temp
        self.level_gases = ([] if level_gas is None else [level_gas]) if level_gases is None else list(level_gases)
        self.gases = ([] if level_gas is None else [gas]) if gases is None else list(gases)
        self.par_lgas = np.zeros(len(par_level), np.int32) if par_lgas is None else par_lgas


class LimbPixel(object):
    """A limb pixel: tangent altitude of its centre LOS, half extent of the FOV in altitude (the lower /
    upper LOS are at alt -+ fov_half: pix.low_LOS() / LOS() / up_LOS(), spect_main_module.py:2704-2706),
    rotation of the square pixel, observation / noise / mask on the low-resolution bands."""

    def __init__(self, limb_tg_alt, fov_half=0.0, pixel_rot=0.0, observation=None, noise=None, mask=None):
        self.limb_tg_alt, self.fov_half, self.pixel_rot = float(limb_tg_alt), float(fov_half), float(pixel_rot)
        self.observation, self.noise, self.mask = observation, noise, mask

    def los_alts(self):
        return [self.limb_tg_alt - self.fov_half, self.limb_tg_alt, self.limb_tg_alt + self.fov_half]


def _ils(scene):
    """The scene's tabulated line shape (None: the Gaussian)."""
    return getattr(scene, "ils", None)


class LimbScene(object):
    """1-D atmosphere on altitude levels z [km] (temps [K], press [hPa]), gases, spectral grid, instrument bands
    (centres / Gaussian sigmas in nm).  ils: an engine.ILS, the bands' tabulated line shape in the Gaussian's place
    (widths_nm then scale its reduced offsets): every band integral of simulate, radtran, inversion_fast_limb, inversion
    and inversion_state, and BandCalibration's two instrument rows, are taken with it.
    sun: a Sun.  With it, the emission rows of every TableGas(solar=...) are thermal + single-scattered sunlight
    (coefficients() ends with one solar pass over the layer rows, solar_pass); the tangent-SZA approximation -- the
    reference's use_tangent_sza = True: mu = cos(sza) on every row -- and Theta = 180 deg - phase.  A per-step SZA is
    the 3-D route: engine.solar_source on geometry.limb_los_3d's rows, and sunlit_steps(L3) makes those rows -- with the
    diffuse field under every step's own SZA (engine.diffuse_source_columns) for a Sun(multiple=True).
    thermal_scattering: a ThermalScattering.  With it every TableGas(solar=...) is a thermal scatterer, with or without a
    sun, and its emission rows are made by thermal_pass: [order-one solar rows +] one engine.diffuse_thermal_source call
    with own_emission=True, which carries beam and sun as well under a Sun(multiple=True).  None runs none of it."""

    def __init__(self, grid, z, temps, press, gases, bands_nm, widths_nm, R=2575.0, n_sub=3, out_units="Wm2", ils=None,
                 sun=None, thermal_scattering=None):
        self.grid = np.asarray(grid, dtype=float)
        self.sun = sun
        self.thermal_scattering = thermal_scattering    # a ThermalScattering: the solar gases are thermal scatterers (thermal_pass)
        if thermal_scattering is not None:
            for g in gases:
                if getattr(g, "solar", None) is not None and g.solar["g"] < -0.5:
                    raise ValueError("thermal_scattering: gas %r has g = %g, the two-stream solve takes g >= -0.5" % (g.name, g.solar["g"]))
                if getattr(g, "solar", None) is not None and not g.source:
                    raise ValueError("thermal_scattering: gas %r is a thermal scatterer, source=False contradicts it" % g.name)
            if sun is not None and getattr(sun, "multiple", False) and sun.surface_albedo != thermal_scattering.surface_albedo:
                raise ValueError("thermal_scattering: its surface_albedo %g and the Sun(multiple=True)'s %g describe one surface"
                                 % (thermal_scattering.surface_albedo, sun.surface_albedo))
        self.solar_frozen = False   # True: solar rows that exist are kept whatever moves -- the linearisation's own assumption,
                                    # for finite differences that are to see what the Jacobians see (a rebuilt thermal pair
                                    # still gets its solar rows again)
        self.keep_solar_rows = False  # True: the solar pass keeps every solar gas's solar rows alone (g.solar_rows), what
                                      # solar_attenuation_jacobian works on (inversion_state(solar_attenuation=True) sets it)
        self.keep_mean_intensity = False  # True: the diffuse pass also keeps its mean intensity J (self.diffuse_J), from the call it
                                          # makes anyway (optics_jacobian's direct part; inversion_state sets it for an "optics" set)
        self.diffuse_J = None
        self.keep_diffuse_state = False  # True: the diffuse pass keeps its inputs (self.diffuse_state), what diffuse_jacobian
                                         # differentiates (inversion_state(diffuse_jacobian=True) sets it)
        self.diffuse_state = None
        if sun is not None and sun.irradiance.shape != self.grid.shape:
            raise ValueError("the sun's irradiance must be given on the scene's grid")
        if sun is not None and getattr(sun, "multiple", False):
            for g in gases:
                if getattr(g, "solar", None) is not None and g.solar["g"] < -0.5:
                    raise ValueError("Sun(multiple=True): gas %r has g = %g, the two-stream solve takes g >= -0.5" % (g.name, g.solar["g"]))
        self.z, self.temps, self.press = (np.asarray(v, dtype=float) for v in (z, temps, press))
        self.nd = syn.number_density(self.press, self.temps)
        # a TableGas with accumulate_into has no slot: it is folded into a line gas's pair (self.folded)
        self.gases = [g for g in gases if getattr(g, "accumulate_into", None) is None]
        self.folded = [g for g in gases if getattr(g, "accumulate_into", None) is not None]
        for t in self.folded:
            host = [g for g in self.gases if g.name == t.accumulate_into]
            if len(host) != 1 or isinstance(host[0], (LevelGas, TableGas)):
                raise ValueError("TableGas %r: accumulate_into=%r names no plain line Gas of the scene" % (t.name, t.accumulate_into))
        self.bands_nm, self.widths_nm = np.asarray(bands_nm, float), np.asarray(widths_nm, float)
        self.bands_nm0, self.widths_nm0 = self.bands_nm.copy(), self.widths_nm.copy()   # the nominal calibration (BandCalibration)
        self.R, self.n_sub, self.out_units = R, n_sub, out_units
        self.ils = ils

    def gas(self, name):
        return [g for g in self.gases if g.name == name][0]

    def coefficients(self, refresh=False, g_lo=0, g_hi=None):
        """(abs, emi) of every gas at the layer stack over grid points [g_lo, g_hi); cached per shard: only VMRs change
        between the iterations of a VMR retrieval (refresh=True recomputes, e.g. when temperatures are retrieved)."""
        g_hi = len(self.grid) if g_hi is None else int(g_hi)
        for g in self.gases:
            if isinstance(g, LevelGas):      # the combine of its resident tables, redone only when its tvib changed
                g.layer_coefficients(self.temps, self.press, g_lo=g_lo, g_hi=g_hi)
                continue
            self.gas_coefficients(g, refresh, g_lo, g_hi)
        self.solar_pass(g_lo, g_hi)
        return [g.coeffs for g in self.gases]

    def solar_gases(self):
        return [g for g in self.gases if getattr(g, "solar", None) is not None] if self.sun is not None else []

    def solar_key(self, g_lo, g_hi):
        """What the solar rows depend on, by content: every gas's VMR profile (and iso_ratio), the identity of every
        gas's absorption table -- temperatures, pressures and vibrational temperatures act through them --, the sun and
        the shard.  A VMR retrieval moves the first and redoes the solar pass each iteration, and nothing else."""
        tabs = tuple(id((g.thermal if getattr(g, "solar", None) is not None else g.coeffs)[0]) for g in self.gases)
        optics = tuple((float(g.solar["albedo"]), float(g.solar["g"])) for g in self.solar_gases())    # (a HazeOptics set moves them)
        return (tuple(np.asarray(g.vmr, float).tobytes() for g in self.gases), tuple(float(g.iso_ratio) for g in self.gases),
                tabs, self.sun.key(), int(g_lo), int(g_hi), optics)

    def solar_weights(self, g, lit):
        """w [n_layers] = albedo P(Theta) / 4 pi of a solar gas, 0 on the rows in shadow."""
        P = geometry.hg_phase(self.sun.cos_scattering, g.solar["g"])
        return np.where(lit, g.solar["albedo"] * P / (4.0 * np.pi), 0.0)

    def shell_midpoints(self):
        """The middles of the shells above the levels z (the last one as thick as the one below it): the points of the
        solar pass's rows."""
        zz = np.append(self.z, self.z[-1] + (self.z[-1] - self.z[-2]))
        return 0.5 * (zz[:-1] + zz[1:])

    def solar_pass(self, g_lo, g_hi):
        """The emission rows of the solar gases: thermal + sca S on the layer rows (engine.solar_source under
        accumulate, on a copy of the cached thermal emi).  The point of a row is the middle of its shell, its columns
        towards the sun geometry.solar_columns with the scene's VMRs.  Held fixed by every Jacobian within one
        linearisation.  The attenuation is the 1-D scene's: a gas whose profile a driver keeps per latitude box
        (inversion_boxes: gas.vmr_boxes) enters it with its 1-D vmr.
        A scene that was asked for the solar rows alone (keep_solar_rows) keeps g.solar_rows = sca S of every solar gas,
        made by an overwrite call, and its emission rows are thermal + those -- the same sum the accumulating call
        forms (solar_attenuation_jacobian's input).  The same rule of when nothing is redone."""
        if self.thermal_scattering is not None:
            return self.thermal_pass(g_lo, g_hi)
        solar = self.solar_gases()
        if not solar:
            return
        import torch
        rows = self.keep_solar_rows
        done = all(g.coeffs is not g.thermal and (not rows or getattr(g, "solar_rows", None) is not None) for g in solar)
        if done and self.solar_frozen:
            return
        key = self.solar_key(g_lo, g_hi) + (("rows",) if rows else ())
        if done and getattr(self, "_solar_key", None) == key:
            return
        U, lit = geometry.solar_columns(self.z, self.nd, [g.vmr for g in self.gases], self.shell_midpoints(), self.sun.mu, R=self.R,
                                        n_sub=self.n_sub, col_scale=[g.iso_ratio for g in self.gases])
        tabs = [(g.thermal if g in solar else g.coeffs)[0] for g in self.gases]
        A = torch.stack(tabs).contiguous()
        sun = torch.as_tensor(self.sun.irradiance[g_lo:g_hi], device="cuda").contiguous()
        for g in solar:
            if rows:
                g.solar_rows = engine.solar_source(A, U, self.solar_weights(g, lit), g.thermal[0], sun)
                emi = g.thermal[1] + g.solar_rows
            else:
                emi = g.thermal[1].clone()
                engine.solar_source(A, U, self.solar_weights(g, lit), g.thermal[0], sun, out=emi, accumulate=True)
            g.coeffs = (g.thermal[0], emi)
        if self.sun.multiple:       # (g.solar_rows stays the single-scattered part alone)
            self.diffuse_pass(solar, A, sun)
        # (the tables themselves are kept beside the key: an id in it stays theirs while they live here.  The key knows a
        # table by identity, as coefficient_stack does: every rebuild in this package makes new tensors; a caller who
        # overwrites a table IN PLACE sets scene._solar_key = None)
        self._solar_key, self._solar_tabs = key, tabs

    def thermal_scatterers(self):
        return [g for g in self.gases if getattr(g, "solar", None) is not None] if self.thermal_scattering is not None else []

    def thermal_pass(self, g_lo, g_hi):
        """The emission rows of the thermal scatterers (thermal_scattering): [order-one solar rows, if a sun] + one
        engine.diffuse_thermal_source call with own_emission=True -- the gas's own emission (1 - albedo) abs B and the
        diffuse field scattered into the line of sight; under a Sun(multiple=True) that call carries beam and sun too, so
        that the layers are walked once for both sources.  With one scatterer the cached thermal emi of the gas is not
        used: the kernel forms B itself.  With several the field is solved once (mean_intensity=True, no rows) and every
        gas gets its order-one rows + (1 - albedo) times its cached thermal emi -- the table's own abs B, the same Planck
        evaluation bit for bit, scaled by Kirchhoff's law: the one place that pair's emi is read -- + one torch.addcmul of
        J with ssa_G (1 - f_G) of the gas's own slot.  Held fixed by every Jacobian within one
        linearisation; the rule of when nothing is redone is solar_pass's (solar_frozen, the key -- which here also
        holds the layer temperatures and the ThermalScattering's values)."""
        scat = self.thermal_scatterers()
        if not scat:
            return
        import torch
        ts, sun = self.thermal_scattering, self.sun
        rows = self.keep_solar_rows and sun is not None
        done = all(g.coeffs is not g.thermal and (not rows or getattr(g, "solar_rows", None) is not None) for g in scat)
        if done and self.solar_frozen:
            return
        tabs = [(g.thermal if g in scat else g.coeffs)[0] for g in self.gases]
        optics = tuple((float(g.solar["albedo"]), float(g.solar["g"])) for g in scat)
        key = (tuple(np.asarray(g.vmr, float).tobytes() for g in self.gases), tuple(float(g.iso_ratio) for g in self.gases),
               tuple(id(t) for t in tabs), None if sun is None else sun.key(), int(g_lo), int(g_hi), optics, self.temps.tobytes(),
               ts.key()) + (("rows",) if rows else ())
        if done and getattr(self, "_solar_key", None) == key:
            return
        A = torch.stack(tabs).contiguous()
        order_one = {}
        sun_t = None
        if sun is not None:     # order one: the single-scattering rows, with the exact phase function and the unscaled beam
            U, lit = geometry.solar_columns(self.z, self.nd, [g.vmr for g in self.gases], self.shell_midpoints(), sun.mu, R=self.R,
                                            n_sub=self.n_sub, col_scale=[g.iso_ratio for g in self.gases])
            sun_t = torch.as_tensor(sun.irradiance[g_lo:g_hi], device="cuda").contiguous()
            for g in scat:
                order_one[g.name] = engine.solar_source(A, U, self.solar_weights(g, lit), g.thermal[0], sun_t)
                if rows:
                    g.solar_rows = order_one[g.name]
        kw = dict(t_surface=0.0 if ts.surface_temperature is None else ts.surface_temperature, surface_albedo=ts.surface_albedo,
                  g_lo=g_lo)
        if sun is not None and sun.multiple:
            V, ssa, asym, beam = self.diffuse_inputs(scat, A, sun_t)
            kw.update(beam=beam, sun=sun_t, mu0=sun.mu)
        else:
            ssa, asym, iso, _, _ = self.diffuse_geometry(scat)
            V = geometry.vertical_columns(self.z, self.nd, [g.vmr for g in self.gases], R=self.R, n_sub=self.n_sub, col_scale=iso)
        if len(scat) == 1:
            g = scat[0]
            emi = order_one.get(g.name)
            if emi is not None and rows:
                emi = emi.clone()
            emi = engine.diffuse_thermal_source(A, V, ssa, asym, self.temps, self.grid, out_gas=self.gases.index(g), out=emi,
                                                accumulate=emi is not None, own_emission=True, **kw)
            g.coeffs = (g.thermal[0], emi)
        else:
            J = engine.diffuse_thermal_source(A, V, ssa, asym, self.temps, self.grid, mean_intensity=True, **kw)
            for g in scat:
                i = self.gases.index(g)
                emi = order_one.get(g.name)
                emi = g.thermal[1] * float(1.0 - ssa[i]) if emi is None else torch.add(emi, g.thermal[1], alpha=float(1.0 - ssa[i]))
                emi.addcmul_(A[i], J, value=float(ssa[i] * (1.0 - max(asym[i], 0.0) ** 2)))
                g.coeffs = (g.thermal[0], emi)
        self._solar_key, self._solar_tabs = key, tabs

    def diffuse_geometry(self, solar):
        """(ssa, asym, iso, pts, beam_scale) of the diffuse pass and of its derivative: per gas slot the single-scattering
        albedo and asymmetry parameter (0 for a gas that is not solar) and the column scale, the points of the direct
        beam (the middles of the shells, then z[0]) and the delta-scaled column scale iso (1 - ssa f) of its columns."""
        ssa = np.array([g.solar["albedo"] if g in solar else 0.0 for g in self.gases])
        asym = np.array([g.solar["g"] if g in solar else 0.0 for g in self.gases])
        iso = np.array([float(g.iso_ratio) for g in self.gases])
        pts = np.append(self.shell_midpoints(), self.z[0])
        return ssa, asym, iso, pts, iso * (1.0 - ssa * np.maximum(asym, 0.0) ** 2)

    def diffuse_inputs(self, solar, A, sun):
        """(V, ssa, asym, beam) of engine.diffuse_source for the scene's state: the layers' vertical columns, the solar
        gases' single-scattering albedos and asymmetry parameters (0 for every other gas) and the direct beam at the
        middles of the shells and at the level z[0] -- one more engine.solar_source(..., transmission=True) call with
        every solar gas's columns scaled by 1 - ssa f, f = max(g, 0)^2: the delta-scaled beam, in spherical geometry."""
        ssa, asym, iso, pts, beam_scale = self.diffuse_geometry(solar)
        vmr = [g.vmr for g in self.gases]
        Ub, lit = geometry.solar_columns(self.z, self.nd, vmr, pts, self.sun.mu, R=self.R, n_sub=self.n_sub, col_scale=beam_scale)
        _, beam = engine.solar_source(A, Ub, np.where(lit, 1.0, 0.0), A[self.gases.index(solar[0])], sun,
                                      src_row=np.zeros(len(pts), np.int32), transmission=True)
        V = geometry.vertical_columns(self.z, self.nd, vmr, R=self.R, n_sub=self.n_sub, col_scale=iso)
        return V, ssa, asym, beam

    def diffuse_pass(self, solar, A, sun):
        """Adds the diffuse rows (Sun(multiple=True)) to the emission rows the solar pass has just made: one
        engine.diffuse_source call -- with one solar gas the fused accumulate, with several the mean intensity once and
        a torch.addcmul per gas."""
        V, ssa, asym, beam = self.diffuse_inputs(solar, A, sun)
        kw = dict(surface_albedo=self.sun.surface_albedo)
        if self.keep_diffuse_state:
            self.diffuse_state = (A, V, ssa, asym, beam, sun)
        if len(solar) == 1:
            if self.keep_mean_intensity:    # (the same kernel with one more store: the rows keep their bits)
                kw["mean_intensity"] = True
            res = engine.diffuse_source(A, V, ssa, asym, beam, sun, self.sun.mu, out_gas=self.gases.index(solar[0]),
                                        out=solar[0].coeffs[1], accumulate=True, **kw)
            self.diffuse_J = res[1] if self.keep_mean_intensity else None
            return
        J = engine.diffuse_source(A, V, ssa, asym, beam, sun, self.sun.mu, mean_intensity=True, **kw)
        self.diffuse_J = J if self.keep_mean_intensity else None
        for g in solar:
            i = self.gases.index(g)
            g.coeffs[1].addcmul_(A[i], J, value=float(ssa[i] * (1.0 - max(asym[i], 0.0) ** 2)))

    def sunlit_steps(self, L3, n_columns=4, g_lo=0, g_hi=None):
        """The per-gas (abs, emi) pairs on the step rows of a 3-D batch L3 (geometry.limb_los_3d), each step under its own
        solar zenith angle L3["seg_mu"]: what engine.limb_rays takes with an engine.LimbLOS of L3.  The layer rows are
        gathered by L3["seg_alt_layer"]; the solar gases' emission is thermal + order one with the per-step SZA (one
        engine.solar_source call per solar gas over the steps, columns towards the sun from the middle of each step).
        With Sun(multiple=True) the diffuse field is added by one engine.diffuse_source_columns call per solar gas under
        accumulate: n_columns solar zenith angles equally spaced in mu over the steps' range (geometry.sza_columns), linear
        in mu between them, the beams of all columns from ONE engine.solar_source(..., transmission=True) call over
        n_columns x (n_layers + 1) points -- diffuse_inputs' points, delta scaling and V.  The sun's sza_deg is not read;
        its phase, irradiance, multiple and surface_albedo are.  Nothing of the scene's own 1-D solar pass is used or
        changed, and no Jacobian is made of these rows."""
        import torch
        solar = self.solar_gases()
        if not solar:
            raise ValueError("sunlit_steps needs a scene with a Sun and a TableGas(solar=...)")
        g_hi = len(self.grid) if g_hi is None else int(g_hi)
        for g in self.gases:        # coefficients() without its solar pass: that one is the tangent-SZA sun's
            if isinstance(g, LevelGas):
                g.layer_coefficients(self.temps, self.press, g_lo=g_lo, g_hi=g_hi)
            else:
                self.gas_coefficients(g, False, g_lo, g_hi)
        pairs = [g.thermal if g in solar else g.coeffs for g in self.gases]
        layer = np.ascontiguousarray(L3["seg_alt_layer"], dtype=np.int32)
        rows = torch.as_tensor(layer.astype(np.int64), device="cuda")
        A = torch.stack([p[0] for p in pairs]).contiguous()
        step_abs = [A[i][rows].contiguous() for i in range(len(pairs))]
        step_emi = [p[1][rows].contiguous() for p in pairs]
        lo, hi = L3["pt_off"][:-1], L3["pt_off"][1:] - 1
        alt_mid = 0.5 * (L3["alt"][(lo + hi) // 2] + L3["alt"][(lo + hi + 1) // 2])
        vmr, iso = [g.vmr for g in self.gases], [g.iso_ratio for g in self.gases]
        U, lit = geometry.solar_columns(self.z, self.nd, vmr, alt_mid, L3["seg_mu"], R=self.R, n_sub=self.n_sub, col_scale=iso)
        sun = torch.as_tensor(self.sun.irradiance[g_lo:g_hi], device="cuda").contiguous()
        for g in solar:
            i = self.gases.index(g)
            engine.solar_source(A, U, self.solar_weights(g, lit), pairs[i][0], sun, src_row=layer, out=step_emi[i], accumulate=True)
        if self.sun.multiple:
            mu_nodes, col_w = geometry.sza_columns(L3["seg_mu"], n_columns)
            ssa, asym, iso_a, pts, beam_scale = self.diffuse_geometry(solar)
            cols = [geometry.solar_columns(self.z, self.nd, vmr, pts, float(m), R=self.R, n_sub=self.n_sub, col_scale=beam_scale)
                    for m in mu_nodes]
            Ub, lit_b = np.concatenate([c[0] for c in cols]), np.concatenate([c[1] for c in cols])
            _, beams = engine.solar_source(A, Ub, np.where(lit_b, 1.0, 0.0), A[self.gases.index(solar[0])], sun,
                                           src_row=np.zeros(len(lit_b), np.int32), transmission=True)
            beams = beams.view(len(mu_nodes), len(pts), -1)
            V = geometry.vertical_columns(self.z, self.nd, vmr, R=self.R, n_sub=self.n_sub, col_scale=iso_a)
            for g in solar:
                i = self.gases.index(g)
                engine.diffuse_source_columns(A, V, ssa, asym, beams, sun, mu_nodes, col_w, layer, surface_albedo=self.sun.surface_albedo,
                                              out_gas=i, out=step_emi[i], accumulate=True)
        return list(zip(step_abs, step_emi))

    def solar_attenuation_jacobian(self, los, alt, w, coeffs, jac=None):
        """The solar attenuation in the column rows of a state Jacobian: d rad / d x_p through tau for the column block
        of the StateWeights `w` (its level masks w.col_masks and gases w.par_gas), added to rows 0 .. n_col - 1 of jac
        [n_rays, n_rows, n_pts] (None: returned as its own [n_rays, n_col, n_pts]).  dU from
        geometry.solar_column_weights at the solar pass's points (the middles of the shells, the tangent-SZA sun), Q by
        ONE limb_rays_layer_jacobian call with dabs = 0 and demi = every solar gas's solar rows, then one fused call
        (engine.solar_attenuation_jacobian).  Needs keep_solar_rows and the solar pass of the current state (`coeffs` is
        coefficient_stack()'s pair); `alt` (the LOS sample altitudes) is not needed: the rows are the scene's layers.
        limb_rays_layer_jacobian is a four-gas call."""
        import torch
        solar = self.solar_gases()
        if not solar or any(getattr(g, "solar_rows", None) is None for g in solar):
            raise ValueError("solar_attenuation_jacobian needs a sun, a solar gas and keep_solar_rows = True before the solar pass")
        n_col = len(w.par_gas)
        if n_col == 0:
            return jac
        dU, _ = geometry.solar_column_weights(self.z, self.nd, w.col_masks, w.par_gas, len(self.gases), self.shell_midpoints(),
                                              self.sun.mu, R=self.R, n_sub=self.n_sub, col_scale=[g.iso_ratio for g in self.gases])
        a, _ = engine.gas_stack(coeffs)
        sol = torch.zeros_like(a)
        for g in solar:
            sol[self.gases.index(g)] = g.solar_rows
        Q = self._emission_rows_jacobian(coeffs, sol, los)
        return self._into_jac(engine.solar_attenuation_jacobian, (a, dU, Q), jac, n_col)

    def diffuse_jacobian(self, los, alt, w, coeffs, jac=None):
        """The diffuse rows in the column rows of a state Jacobian: d rad / d x_p through the two-stream solve of the
        diffuse pass (Sun(multiple=True)) for the column block of the StateWeights `w`, added to rows 0 .. n_col - 1 of jac
        [n_rays, n_rows, n_pts] (None: returned as its own [n_rays, n_col, n_pts]).  dV from
        geometry.vertical_column_weights; the beam's part from geometry.solar_column_weights at diffuse_inputs' points
        (the middles of the shells and z[0]) with its delta-scaled col_scale, dlnbeam = -(dUb . A) as one torch.matmul
        (rows in shadow are zero); Q by ONE limb_rays_layer_jacobian call with dabs = 0 and demi[g] = ssa_g (1 - f_g) A[g]
        of every solar gas -- the radiances' derivative to J; then one engine.diffuse_jacobian call.  Needs
        keep_diffuse_state and the solar pass of the current state (V, ssa, asym and beam are that pass's own; `coeffs` is
        coefficient_stack()'s pair); `alt` is not needed: the rows are the scene's layers.  The derivative through the
        single-scattering rows' own optical depth is solar_attenuation_jacobian's: the full derivative of a sunlit
        multiple-scattering scene is both.  limb_rays_layer_jacobian is a four-gas call."""
        import torch
        solar = self.solar_gases()
        _refuse_thermal_scattering(self, "diffuse_jacobian")
        state = self.diffuse_state
        if not solar or not getattr(self.sun, "multiple", False) or state is None:
            raise ValueError("diffuse_jacobian needs a Sun(multiple=True), a solar gas and keep_diffuse_state = True before the solar pass")
        n_col = len(w.par_gas)
        if n_col == 0:
            return jac
        A, V, ssa, asym, beam, sun = state
        n_gas, n_layers, n_pts = (int(v) for v in A.shape)
        _, _, iso, pts, beam_scale = self.diffuse_geometry(solar)
        f = np.maximum(asym, 0.0) ** 2
        dV = geometry.vertical_column_weights(self.z, self.nd, w.col_masks, w.par_gas, n_gas, R=self.R, n_sub=self.n_sub, col_scale=iso)
        dUb, _ = geometry.solar_column_weights(self.z, self.nd, w.col_masks, w.par_gas, n_gas, pts, self.sun.mu, R=self.R,
                                               n_sub=self.n_sub, col_scale=beam_scale)
        dub = torch.as_tensor(np.ascontiguousarray(dUb.reshape(n_col * (n_layers + 1), n_gas * n_layers)), device="cuda")
        dlnbeam = torch.matmul(dub, A.reshape(n_gas * n_layers, n_pts)).neg_().reshape(n_col, n_layers + 1, n_pts)
        W = torch.zeros_like(A)
        for g in solar:
            i = self.gases.index(g)
            W[i] = A[i] * float(ssa[i] * (1.0 - f[i]))
        Q = self._emission_rows_jacobian(coeffs, W, los)
        return self._into_jac(engine.diffuse_jacobian, (A, V, ssa, asym, beam, sun, self.sun.mu, dV, dlnbeam, Q), jac, n_col,
                              surface_albedo=self.sun.surface_albedo)

    def optics_jacobian(self, los, alt, params, coeffs):
        """[n_rays, n_opt, n_pts]: the complete derivative of the radiances to the optics parameters `params` (HazeOptics.keys:
        ("albedo", gas), ("g", gas), ("surface_albedo", None)) at the current state, the sum of three parts.
        Direct: the emission rows' own coefficients move with J and the beam held -- per parameter the order-one rows with
        d w in place of w (ONE engine.solar_source call: no division by w, rows in shadow stay exact zeros), plus
        d(ssa (1 - f)) A[g] J of the diffuse rows (keep_mean_intensity: J from the diffuse pass's own call), pushed
        through one _emission_rows_jacobian call and summed over the layers.  Beam: d ln beam = -(dUb . A), dUb the
        delta-scaled beam's columns scaled, after solar_columns (the sign is negative), by d(1 - ssa f) / d x of the
        parameter's gas; one torch.matmul.  Two-stream: ONE engine.diffuse_optics_jacobian call with diffuse_jacobian's Q.
        With Sun(multiple=False) only the direct part exists and a surface_albedo parameter is refused.  `alt` is not
        needed.  limb_rays_layer_jacobian is a four-gas call."""
        import torch
        solar = self.solar_gases()
        _refuse_thermal_scattering(self, "optics_jacobian (a HazeOptics set)")
        multiple = bool(getattr(self.sun, "multiple", False))
        params = list(params)
        if not solar or not params:
            raise ValueError("optics_jacobian needs a sun, a solar gas and at least one parameter")
        for kind, gas in params:
            if kind == "surface_albedo":
                if not multiple:
                    raise ValueError("a surface_albedo parameter needs a Sun(multiple=True): single scattering does not see the ground")
            elif kind not in ("albedo", "g") or gas not in [g.name for g in solar]:
                raise ValueError("optics parameter %r: albedo or g of a solar gas, or surface_albedo" % ((kind, gas),))
        if multiple and (self.diffuse_state is None or self.diffuse_J is None):
            raise ValueError("optics_jacobian needs keep_diffuse_state = keep_mean_intensity = True before the solar pass")
        n_gas, n_opt = len(self.gases), len(params)
        ssa, asym, iso, pts, _ = self.diffuse_geometry(solar)
        pos = np.maximum(asym, 0.0)
        f = pos ** 2
        dssa, dasym, dalb = np.zeros((n_opt, n_gas)), np.zeros((n_opt, n_gas)), np.zeros(n_opt)
        for p, (kind, gas) in enumerate(params):
            if kind == "surface_albedo":
                dalb[p] = 1.0
            else:
                (dssa if kind == "albedo" else dasym)[p, self.gases.index(self.gas(gas))] = 1.0
        dcs = dssa * (1.0 - f) - ssa * 2.0 * pos * dasym                       # d(ssa (1 - f)) [n_opt, n_gas]
        a, _ = engine.gas_stack(coeffs)
        n_layers, n_pts = int(a.shape[1]), int(a.shape[2])
        sun = torch.as_tensor(self.sun.irradiance[self._solar_key[4]:self._solar_key[5]], device="cuda").contiguous()
        tabs = torch.stack([(g.thermal if g in solar else g.coeffs)[0] for g in self.gases]).contiguous()
        U, lit = geometry.solar_columns(self.z, self.nd, [g.vmr for g in self.gases], self.shell_midpoints(), self.sun.mu, R=self.R,
                                        n_sub=self.n_sub, col_scale=[g.iso_ratio for g in self.gases])
        P = {g.name: (geometry.hg_phase(self.sun.cos_scattering, g.solar["g"]), geometry.hg_phase_dg(self.sun.cos_scattering, g.solar["g"]))
             for g in solar}
        direct = []
        for p, (kind, gas) in enumerate(params):
            if kind == "surface_albedo":
                direct.append(None)
                continue
            g = self.gas(gas)
            i = self.gases.index(g)
            dw = P[gas][0] if kind == "albedo" else g.solar["albedo"] * P[gas][1]
            demi = torch.zeros_like(a)
            # (the entry takes weights >= 0 and d P / d g has either sign: the rows are linear in the one weight, so its
            # magnitude goes in and its sign onto the rows)
            demi[i] = engine.solar_source(tabs, U, np.where(lit, abs(dw) / (4.0 * np.pi), 0.0), g.thermal[0], sun)
            if dw < 0.0:
                demi[i].neg_()
            if multiple and dcs[p, i] != 0.0:
                demi[i].addcmul_(tabs[i], self.diffuse_J, value=float(dcs[p, i]))
            direct.append(self._emission_rows_jacobian(coeffs, demi, los).sum(dim=1))
        n_rays = next(d.shape[0] for d in direct if d is not None) if any(d is not None for d in direct) else None
        if multiple:
            A, V, ssa_s, asym_s, beam, sun_s = self.diffuse_state
            Ub, litb = geometry.solar_columns(self.z, self.nd, [g.vmr for g in self.gases], pts, self.sun.mu, R=self.R, n_sub=self.n_sub,
                                              col_scale=iso)
            dscale = -(dssa * f + ssa * 2.0 * pos * dasym)                     # d(1 - ssa f) / d x_p [n_opt, n_gas]
            dUb = dscale[:, None, :, None] * (Ub * np.asarray(litb, float)[:, None, None])[None]
            dub = torch.as_tensor(np.ascontiguousarray(dUb.reshape(n_opt * (n_layers + 1), n_gas * n_layers)), device="cuda")
            dlnbeam = torch.matmul(dub, A.reshape(n_gas * n_layers, n_pts)).neg_().reshape(n_opt, n_layers + 1, n_pts)
            W = torch.zeros_like(A)
            for g in solar:
                i = self.gases.index(g)
                W[i] = A[i] * float(ssa[i] * (1.0 - f[i]))
            Q = self._emission_rows_jacobian(coeffs, W, los)
            out = engine.diffuse_optics_jacobian(A, V, ssa_s, asym_s, beam, sun_s, self.sun.mu, dssa, dasym, dalb, dlnbeam, Q,
                                                 surface_albedo=self.sun.surface_albedo)
        else:
            out = torch.zeros((n_rays, n_opt, n_pts), dtype=torch.float64, device="cuda")
        for p, d in enumerate(direct):
            if d is not None:
                out[:, p] += d
        return out

    @staticmethod
    def _emission_rows_jacobian(coeffs, demi, los):
        """Q [n_rays, n_layers, n_pts]: the radiances' derivative to a factor on the rows demi [n_gas, n_layers, n_pts] of
        the emission, the absorption held: ONE limb_rays_layer_jacobian call with dabs = 0."""
        import torch
        return engine.limb_rays_layer_jacobian(coeffs, (torch.zeros_like(demi), demi), los)

    @staticmethod
    def _into_jac(fused, args, jac, n_col, **kw):
        """fused(*args) as its own [n_rays, n_col, n_pts] (jac None), or added to rows 0 .. n_col - 1 of jac."""
        if jac is None:
            return fused(*args, **kw)
        return fused(*args, out=jac, par_slot=np.arange(n_col), accumulate=True, **kw)

    def folded_into(self, g):
        return [t for t in self.folded if t.accumulate_into == g.name]

    def gas_coefficients(self, g, refresh, g_lo, g_hi):
        """(abs, emi) of a TableGas or a plain line Gas over [g_lo, g_hi), kept on the gas; a line gas's pair has the
        tables folded into it (accumulate_into) added, and is rebuilt when one of them moved."""
        if isinstance(g, TableGas):
            return g.layer_coefficients(self, g_lo=g_lo, g_hi=g_hi)
        fkey = tuple(t.cache_key(self, g_lo, g_hi) for t in self.folded_into(g))
        if g.coeffs is None or refresh or getattr(g, "coeffs_shard", None) != (g_lo, g_hi) or getattr(g, "_folded_key", ()) != fkey:
            g.set_self_pressure(self.press)
            g.coeffs = g.lineset.abscoeff_layers(self.temps, self.press, tvib=g.tvib, g_lo=g_lo, g_hi=g_hi)
            g.coeffs_shard, g._folded_key = (g_lo, g_hi), fkey
            for t in self.folded_into(g):
                t.table.layers(self.temps, self.grid, press=self.press, scale=t.scale_of(self), source=t.source, g_lo=g_lo,
                               g_hi=g_hi, out=g.coeffs, accumulate=True)
        return g.coeffs

    def coefficient_stack(self, refresh=False, g_lo=0, g_hi=None):
        """coefficients() as the stacked pair the limb_rays* calls work on (engine.gas_stack), re-stacked only when a
        gas's tables were recomputed: a VMR retrieval passes the same tables in every iteration."""
        co = self.coefficients(refresh=refresh, g_lo=g_lo, g_hi=g_hi)
        key = tuple(id(c[0]) for c in co) + tuple(id(c[1]) for c in co)
        if getattr(self, "_stack_key", None) != key:
            self._stack, self._stack_key = engine.gas_stack(co), key
            self._stack_of = co          # keeps the ids alive
        return self._stack

    def los(self, tangent_alts, update=True, path=False, **opts):
        """engine.LimbLOS of rays with the given tangent altitudes (photon order) + the sample altitudes.  The geometry
        (paths, sample points, densities) depends on the altitudes alone and is kept; between the iterations of a
        retrieval only the VMRs at the sample points change.  path=True: the batch carries the path derivatives to the
        rays' tangent altitudes (geometry.limb_los(path=True)), which the calls with pointing=True need."""
        # (the key holds everything the geometry is made from: altitudes of the rays, the level grid, the densities, the
        # sub-stepping and the radius -- by content)
        key = (tuple(float(a) for a in tangent_alts), np.asarray(self.z, float).tobytes(), np.asarray(self.nd, float).tobytes(),
               int(self.n_sub), float(self.R)) + ((True,) if path else ())
        geo = getattr(self, "_los_geo", None)
        if geo is None or geo[0] != key:
            L = syn.limb_los(self.z, self.nd, [g.vmr for g in self.gases], tangent_alts, R=self.R, n_sub=self.n_sub,
                             **(dict(path=True) if path else {}))
            top = self.z[-1] + (self.z[-1] - self.z[-2])
            geo = self._los_geo = (key, L, np.append(self.z, top))
        _, L, zz = geo
        # the batch itself is kept too (photon order, no options): its device-resident form (engine.LimbLOS.handle_par)
        # then needs only the new VMRs (LimbLOS.set_vmr: one small copy + the column kernel) -- or nothing at all
        # (update=False) when the caller sets them on the device from the parameter vector (engine.retrieval_forward)
        kept = getattr(self, "_los_obj", None)
        if not update and not opts and kept is not None and kept[0] == key:
            return kept[1], L["alt"]
        # (geometry._profiles: every VMR linear in altitude between the levels, constant above the last one)
        vmr = np.array([np.interp(L["alt"], zz, np.append(g.vmr, g.vmr[-1])) for g in self.gases])
        if not opts and kept is not None and kept[0] == key:
            kept[1].set_vmr(vmr)
            return kept[1], L["alt"]
        los = engine.LimbLOS(L["seg_off"], L["seg_layer"], L["pt_off"], L["x"], L["nd"], vmr,
                             col_scale=[g.iso_ratio for g in self.gases],
                             path=dict(alt=L["alt"], dx=L["dx_dzt"], dalt=L["dalt_dzt"]) if path else None, **opts)
        if not opts:
            self._los_obj = (key, los)
        return los, L["alt"]

    def profile_weights(self, bayes_set, alt):
        """par_gas [n_par], par_w [n_par, n_pt]: the masks of every retrieved parameter at the LOS sample
        altitudes (masks are piecewise linear on the altitude levels, like the VMR between them)."""
        # masks and sample altitudes do not change between the iterations of a retrieval
        params = list(bayes_set.params())
        key = (tuple(np.asarray(par.maskgrid.mask, dtype=float).tobytes() for par in params), tuple(par.nameset for par in params), alt.tobytes())
        cached = getattr(self, "_weights_cache", None)
        if cached is not None and cached[0] == key:
            return cached[1], cached[2]
        names = [g.name for g in self.gases]
        top = self.z[-1] + (self.z[-1] - self.z[-2])
        zz = np.append(self.z, top)
        par_gas, par_w = [], []
        for par in params:
            par_gas.append(names.index(par.nameset))
            m = np.asarray(par.maskgrid.mask, dtype=float)
            par_w.append(np.interp(alt, zz, np.append(m, m[-1])))
        out = (np.array(par_gas, np.int32), np.array(par_w))
        for a in out:
            a.setflags(write=False)     # shared with every caller until the masks change: engine keys resident batches on them
        self._weights_cache = (key, out[0], out[1])
        return out

    def state_weights(self, bayes_set, alt, several_level_gases=False):
        """The parameters of a mixed state vector, split in BayesSet order into the column block -- sets named after a gas:
        VMR-profile parameters, their masks at the LOS sample altitudes `alt` as in profile_weights -- and the level block
        -- sets named "tvib:<gas>:<level>" (TvibProfile) of ONE LevelGas: their masks on the coefficient rows, the scene's
        altitude levels -- and the row block -- the set named "temp" (TempProfile): its masks on the coefficient rows
        likewise.  Returns a StateWeights (its perm leads back to BayesSet order).
        several_level_gases=True: Tvib sets of any number of LevelGas (the calls with level_gases take them in one pass);
        the level block then holds them all in BayesSet order, StateWeights.level_gases / gases / par_lgas say whose each
        is, level_gas / gas are the first one's.  With one LevelGas the result is the same either way.
        The sets named "instr" (BandCalibration) and "pointing" (Pointing) are accepted and have no part in any block: perm
        then covers the other sets' parameters alone, in BayesSet order."""
        names = [g.name for g in self.gases]
        top = self.z[-1] + (self.z[-1] - self.z[-2])
        zz = np.append(self.z, top)
        par_gas, par_w_col, par_level, par_w_lev, par_w_temp, kind, col_masks = [], [], [], [], [], [], []
        level_gas, level_gases, par_lgas = None, [], []
        for name in bayes_set.order:
            st = bayes_set.sets[name]
            if name in (INSTR_SET, POINTING_SET, OPTICS_SET) and name not in names:    # ("optics", HazeOptics, likewise)
                continue
            if name in names:
                for par in st.set:
                    m = np.asarray(par.maskgrid.mask, dtype=float)
                    par_gas.append(names.index(name))
                    par_w_col.append(np.interp(alt, zz, np.append(m, m[-1])))
                    col_masks.append(m)
                    kind.append(0)
                continue
            if name == "temp":
                for par in st.set:
                    m = np.asarray(par.maskgrid.mask, dtype=float)
                    if m.shape != self.z.shape:
                        raise ValueError("the masks of %r are not on the scene's altitude levels" % (name,))
                    par_w_temp.append(m)
                    kind.append(2)
                continue
            parts = name.split(":")
            ok = len(parts) == 3 and parts[0] == "tvib" and parts[1] in names and parts[2].isdigit()
            gas = self.gas(parts[1]) if ok else None
            if not ok or not isinstance(gas, LevelGas) or int(parts[2]) >= gas.n_levels:
                raise ValueError("retrieval set %r names neither a gas of the scene nor tvib:<LevelGas>:<level> with a level "
                                 "of that gas" % (name,))
            if level_gas is not None and gas is not level_gas and not several_level_gases:
                raise ValueError("vibrational-temperature sets of more than one gas (%s, %s): one call has one "
                                 "level-factored gas" % (level_gas.name, gas.name))
            level_gas = gas if level_gas is None else level_gas
            if not any(gas is g for g in level_gases):
                level_gases.append(gas)
            for par in st.set:
                par_lgas.append([gas is g for g in level_gases].index(True))
                m = np.asarray(par.maskgrid.mask, dtype=float)
                if m.shape != self.z.shape:
                    raise ValueError("the masks of %r are not on the scene's altitude levels" % (name,))
                par_level.append(int(parts[2]))
                par_w_lev.append(m)
                kind.append(1)
        kind = np.array(kind, dtype=int)
        n_col = int((kind == 0).sum())
        perm = np.where(kind == 0, np.cumsum(kind == 0) - 1, n_col + np.cumsum(kind == 1) - 1).astype(int)
        if par_w_temp:
            perm = np.where(kind == 2, n_col + len(par_level) + np.cumsum(kind == 2) - 1, perm).astype(int)
        sw = StateWeights(np.array(par_gas, np.int32), np.array(par_w_col, dtype=float).reshape(n_col, len(alt)), level_gas,
                          None if level_gas is None else self.gases.index(level_gas), np.array(par_level, np.int32),
                          np.array(par_w_lev, dtype=float).reshape(len(par_level), len(self.z)), perm,
                          np.array(par_w_temp, dtype=float).reshape(len(par_w_temp), len(self.z)), level_gases,
                          [self.gases.index(g) for g in level_gases], np.array(par_lgas, np.int32))
        sw.col_masks = np.array(col_masks, dtype=float).reshape(n_col, len(self.z))   # the column block's masks on the levels
        return sw

    def temperature_derivatives(self):
        """(coeffs, dcoeffs): (abs, emi) of every gas at the CURRENT temperatures and their derivatives with respect to
        each layer's kinetic temperature (pressure and vibrational temperatures fixed), recomputed for a gas only when
        the temperatures moved since its last call here.  A LevelGas (built with dT) gives both from its pair tables
        (layer_coefficients(derivative=True)); a plain Gas costs two coefficient ops (engine.coefficients_dT, scheme
        "forward", on the coefficients just computed); a TableGas gives its analytic derivatives with its pair, in one
        launch, and the tables folded into a plain Gas add theirs to that gas's two pairs."""
        _refuse_thermal_scattering(self, "temperature_derivatives (a TempProfile set)")
        n_grid = len(self.grid)
        for g in self.gases:
            key = (self.temps.tobytes(), self.press.tobytes()) + tuple(t.cache_key(self, 0, n_grid) for t in self.folded_into(g))
            if isinstance(g, TableGas):
                g.layer_coefficients(self, g_lo=0, g_hi=n_grid, derivative=True)
            elif isinstance(g, LevelGas):
                if not g.dT:
                    raise ValueError("a temperature retrieval needs LevelGas(%r, ..., dT=...): the tables at T + dT" % (g.name,))
                g.layer_coefficients(self.temps, self.press, g_lo=0, g_hi=len(self.grid), derivative=True)   # (coefficients()' own shard key)
            elif getattr(g, "_dT_key", None) != key or g.coeffs is None or g.coeffs_shard != (0, len(self.grid)):
                g.set_self_pressure(self.press)
                g.coeffs = g.lineset.abscoeff_layers(self.temps, self.press, tvib=g.tvib)
                g.coeffs_shard = (0, len(self.grid))
                _, g.dcoeffs = engine.coefficients_dT(g.lineset, self.temps, self.press, tvib=g.tvib, scheme="forward",
                                                      coeffs=g.coeffs)
                g._dT_key, g._folded_key = key, key[2:]
                for t in self.folded_into(g):
                    t.table.layers(self.temps, self.grid, press=self.press, scale=t.scale_of(self), source=t.source,
                                   derivative=True, out=(g.coeffs, g.dcoeffs), accumulate=True)
        self.solar_pass(0, n_grid)      # (the solar rows are held fixed under d / dT: dcoeffs stay the thermal pair's)
        return [g.coeffs for g in self.gases], [g.dcoeffs for g in self.gases]


def _one_call_eligible(pixels, bayes_set, fov_closed_form):
    """The one-call routes (engine.retrieval_forward / retrieval_step) take: every pixel with the closed-form field of view
    or none with one, every retrieved set a linear altitude profile (its VMR at a sample point is sum_p x_p w_p)."""
    with_fov = sum(pix.fov_half > 0 for pix in pixels)
    return ONE_CALL and bayes_set is not None and (with_fov == 0 or (with_fov == len(pixels) and fov_closed_form)) and \
        all(type(st) in (smm.LinearProfile_1D_new, smm.LinearProfile_1D) for st in bayes_set.sets.values())


def _one_call_batch(scene, pixels, bayes_set, alts, with_fov):
    """The resident LOS batch, the parameter weights and the pixels' FOV factors (scene._fov_fac) of a one-call forward
    model.  The gases WITHOUT parameters keep the VMRs the batch was last given: pushed again when one of them got a new
    profile (by CONTENT: an id() can be re-used by a new array and says nothing about an in-place edit)."""
    fixed = tuple(np.asarray(g.vmr, float).tobytes() for g in scene.gases if g.name not in bayes_set.sets)
    stale = getattr(scene, "_los_obj", None) is None or getattr(scene, "_fixed_vmr_key", None) != fixed
    scene._fixed_vmr_key = fixed
    los, alt = scene.los(alts, update=stale)
    par_gas, par_w = scene.profile_weights(bayes_set, alt)
    rots = tuple(pix.pixel_rot for pix in pixels)
    if with_fov and getattr(scene, "_fov_key", None) != rots:
        scene._fov_key, scene._fov_fac = rots, engine.fov_factors(rots)
    return los, par_gas, par_w


def shard_with_halo(n_grid, g_lo, g_hi):
    """Grid range a rank evaluates for its spectral shard [g_lo, g_hi) of an instrument-band integral: one point
    beyond its upper end, so that the trapezoid between the last own point and the next rank's first is counted
    exactly once (every interval (j, j + 1) belongs to the shard that owns j)."""
    return int(g_lo), int(min(g_hi + 1, n_grid))


def los_tags(n_los):
    """Tags of the simulated lines of sight, in the order they are simulated (three per pixel, or the ladder's with
    group_observations): the keys of radtrans and of every single_rads entry."""
    return ['LOS%02d' % i for i in range(n_los)]


def _level_index(lev):
    """A tracked level as an index: an integer, or the reference's level name 'lev_NN'."""
    if isinstance(lev, str):
        if not lev.startswith('lev_'):
            raise ValueError("a level is an index or 'lev_NN', not %r" % (lev,))
        return int(lev[4:])
    return int(lev)


def single_rad_keys(gases, track_levels=None):
    """[(key, gas index, level index | None)]: the entries of single_rads in the reference's order
    (spect_main_module.py:3179-3187): (gas.name, 'iso_<n>') for every gas, followed by (gas.name, 'iso_<n>', lev) for
    each of its tracked levels -- lev as given in track_levels[(gas.name, 'iso_<n>')], an index or 'lev_NN'.
    ValueError for a track_levels key that names no gas of the scene and for a level the gas does not have."""
    track_levels = dict(track_levels or {})
    out = []
    for gi, g in enumerate(gases):
        # (a TableGas has no isotopologue and no levels: 'iso_0', and any tracked level of it is refused below)
        table = isinstance(g, TableGas)
        gasiso = (g.name, 'iso_%d' % (0 if table else g.lineset.iso))
        out.append((gasiso, gi, None))
        n_lev = 0 if table else len(g.lineset.level_energies)
        for lev in track_levels.pop(gasiso, ()):
            L = _level_index(lev)
            if not 0 <= L < n_lev:
                raise ValueError('level {} is not a level of gas {}'.format(lev, g.name))
            out.append((gasiso + (lev,), gi, L))
    if track_levels:
        raise ValueError('track_levels names unknown gases: {}'.format(sorted(track_levels)))
    return out


def pack_single_rads(keys, tags, low, bands_nm):
    """(radtrans, single_rads) of the reference's return (spect_main_module.py:3287) from the low-resolution rows
    low [1 + n_keys, n_los, n_bands]: row 0 the radiances, row 1 + i the part of keys[i] (single_rad_keys)."""
    low = np.asarray(low, dtype=float)
    if low.shape[:2] != (1 + len(keys), len(tags)):
        raise ValueError("low must be [1 + n_keys, n_los, n_bands]")
    radtrans = dict((tag, Spectrum(low[0, i], bands_nm)) for i, tag in enumerate(tags))
    single_rads = dict()
    for k, (key, _, _) in enumerate(keys):
        single_rads[key] = dict((tag, Spectrum(low[1 + k, i], bands_nm)) for i, tag in enumerate(tags))
    return radtrans, single_rads


def _all_reduce_sum(a):
    """The sum of a numpy array over the ranks of a sharded run (distributed.all_reduce_sum: a no-op without a process
    group), through the device under NCCL."""
    import torch
    from . import distributed as sd
    dev = "cuda" if (torch.distributed.is_initialized() and torch.distributed.get_backend() == "nccl") else "cpu"
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sd.all_reduce_sum(t)
    return t.cpu().numpy()


def _ladder(pixels, alts, group):
    """(the tangent altitudes to simulate, the pixels' own `alts` to spline back to | None): with group = (alt_step_sims,
    alt_first_los) the ladder of smm.make_group_observations, otherwise `alts` themselves."""
    if group is None:
        return alts, None
    alts_sim, _ = smm.make_group_observations(list(pixels), alt_step=group[0], alt_first_los=group[1])
    return [float(a) for a in alts_sim], alts


def _closed_form_fov(pixels, fov_closed_form, who):
    """The number of pixels with a field of view; `who` refuses pixels of which only some have one, or any without the
    closed form."""
    with_fov = sum(pix.fov_half > 0 for pix in pixels)
    if not (with_fov == 0 or (with_fov == len(pixels) and fov_closed_form)):
        raise ValueError("%s needs the closed-form field of view for every pixel, or for none" % who)
    return with_fov


def _simulate_budget(scene, pixels, track_levels, fov_closed_form, shard, refresh, group):
    """simulate() with the radiance budget: (sims, radtrans, single_rads).  A gas with tracked levels takes the
    level-factored route (engine.LevelFactored on the scene's layers, kept on the gas per spectral shard; coefficients
    from its steps()), so that its pair tables serve the level parts; one engine.limb_rays_parts call per such gas -- the
    first one also carries the gas parts and the radiances --, one instrument step on the stacked buffer and, with a
    spectral shard, one all-reduce of the partial band integrals of radiances and parts together."""
    import torch
    alts, alts_pix = _ladder(pixels, [a for pix in pixels for a in pix.los_alts()], group)
    keys = single_rad_keys(scene.gases, track_levels)
    n_grid, n_layers, n_gas = len(scene.grid), len(scene.temps), len(scene.gases)
    g_lo, g_hi = (0, n_grid) if shard is None else shard_with_halo(n_grid, *shard)
    rows = np.arange(n_layers, dtype=np.int32)
    tracked = sorted(set(gi for _, gi, L in keys if L is not None))
    coeffs = []
    for gi, g in enumerate(scene.gases):
        if gi in tracked:
            lf = getattr(g, "level_factored", None)
            if lf is None or refresh or g.level_factored_shard != (g_lo, g_hi):
                _refuse_table_gas(g, "the level-factored route of the radiance budget")
                g.set_self_pressure(scene.press)
                lf = g.level_factored = engine.LevelFactored(g.lineset, scene.temps, scene.press, g_lo=g_lo, g_hi=g_hi)
                g.level_factored_shard = (g_lo, g_hi)
            coeffs.append(lf.steps(rows, tvib=g.tvib))
        else:
            coeffs.append(scene.gas_coefficients(g, refresh, g_lo, g_hi))   # (a TableGas is a ('gas', g) part like any other)
    stack = engine.gas_stack(coeffs)
    los, _ = scene.los(alts)
    n_los = len(alts)
    # row k of the stacked buffer: 0 the radiances, 1 + i the part of keys[i]
    buf = [None] * (1 + len(keys))
    gas_rows = [k for k, (_, gi, L) in enumerate(keys) if L is None]
    calls = tracked if tracked else [None]
    for num, gi in enumerate(calls):
        lev_rows = [k for k, (_, gj, L) in enumerate(keys) if L is not None and gj == gi]
        levels = [keys[k][2] for k in lev_rows]
        if gi is None:
            rad, parts = engine.limb_rays_parts(stack, los, np.arange(n_gas), np.full(n_gas, -1), grid=scene.grid, g_lo=g_lo)
        else:
            rad, parts, _ = scene.gases[gi].level_factored.level_radiances(
                stack, los, rows, scene.gases[gi].tvib, levels=levels, gas=gi, grid=scene.grid, gas_parts=num == 0)
        for i, k in enumerate(lev_rows):
            buf[1 + k] = parts[:, i]
        if num == 0:
            buf[0] = rad
            for g, k in enumerate(gas_rows):
                buf[1 + k] = parts[:, len(lev_rows) + g]
    hires = torch.stack(buf).reshape(len(buf) * n_los, -1)
    low = engine.hires_to_lowres(hires, scene.grid, scene.bands_nm, scene.widths_nm, out_units=scene.out_units, g_lo=g_lo,
                                 ils=_ils(scene))
    low = np.asarray(low).reshape(len(buf), n_los, -1)
    if shard is not None:
        low = _all_reduce_sum(low)
    radtrans_, single_rads = pack_single_rads(keys, los_tags(n_los), low, scene.bands_nm)
    at = low[0]
    if alts_pix is not None:
        f = smm.make_radtran_spline(alts, np.ascontiguousarray(low[0]))
        at = np.array([f(a) for a in alts_pix])
    sims = []
    for i, pix in enumerate(pixels):
        three = [Spectrum(at[3 * i + q], scene.bands_nm) for q in range(3)]
        sims.append(smm.FOV_integr_1D(three, pix.pixel_rot, closed_form=fov_closed_form) if pix.fov_half > 0 else three[1])
    return sims, radtrans_, single_rads


def simulate(scene, pixels, bayes_set=None, fov_closed_form=True, shard=None, refresh=False, arrays=False, group=None,
             track_levels=None, full_output=False):
    """One forward-model pass for all pixels (the body of the reference's iteration,
    spect_main_module.py:2736-2940): returns (sims, derivs) with sims[i] the FOV-integrated low-resolution
    spectrum of pixel i (Spectrum) and derivs[i][p] its derivative w.r.t. parameter p of bayes_set.

    shard = (g_lo, g_hi): this rank's spectral window of a multi-GPU run -- the reference splits the forward model
    of a retrieval the same way (spect_main_module.py:2814-2818: n_split contiguous chunks of the grid, results
    put together before the instrument step).  The rank computes radiances and Jacobians on its shard only and its
    PARTIAL instrument-band integrals; one all-reduce (sum) of [n_los x (1 + n_par) x n_bands] doubles over the
    ranks completes them (distributed.all_reduce_sum; a no-op without a process group), then every rank holds the
    same low-resolution spectra and runs the same n_par x n_par algebra.

    arrays=True (every pixel with a field of view and the closed form -- or none with a field of view): returns
    (low [n_pix, n_bands], dlow [n_pix, n_par, n_bands]) instead of the spectrum objects (the retrieval loop: the
    objects of an iteration were ~0.1 ms of its 0.65).

    group = (alt_step_sims, alt_first_los): the reference's group_observations route (spect_main_module.py:2668-2670,
    2908-2930, 3056-3058, 3263-3273) -- the forward model runs on a regular ladder of tangent altitudes
    (smm.make_group_observations) instead of three LOS per pixel, and the pixels' LOS spectra (and derivatives) are read
    off quadratic splines in tangent altitude (smm.make_radtran_spline) before the FOV integration.

    track_levels / full_output (simulation only: bayes_set None): returns (sims, radtrans, single_rads) as the
    reference's radtrans (spect_main_module.py:3287) -- see radtrans below.

    A bayes_set with the "instr" set (BandCalibration) is refused: the one-call forward model behind this function
    (sr_retrieval_forward_dev, and the step and loop calls built on it) has no instrument rows; inversion_state has."""
    _refuse_instr(bayes_set, "simulate (sr_retrieval_forward_dev / _step_dev / _loop_dev)")
    if bayes_set is not None or track_levels is not None or full_output:
        _refuse_many_slots(scene, "simulate with a bayes_set" if bayes_set is not None else "simulate (radiance budget)")
    if track_levels is not None or full_output:
        if bayes_set is not None or arrays:
            raise ValueError("the radiance budget (track_levels / full_output) is a simulation: no bayes_set, no arrays")
        return _simulate_budget(scene, pixels, track_levels, fov_closed_form, shard, refresh, group)
    alts, alts_pix = _ladder(pixels, [a for pix in pixels for a in pix.los_alts()], group)
    n_grid = len(scene.grid)
    g_lo, g_hi = (0, n_grid) if shard is None else shard_with_halo(n_grid, *shard)
    coeffs = scene.coefficient_stack(refresh=refresh, g_lo=g_lo, g_hi=g_hi)
    n_los = len(alts)
    lowres = lambda r: engine.hires_to_lowres(r, scene.grid, scene.bands_nm, scene.widths_nm, out_units=scene.out_units, g_lo=g_lo,
                                              ils=_ils(scene))
    with_fov = sum(pix.fov_half > 0 for pix in pixels)
    if arrays and group is None and _one_call_eligible(pixels, bayes_set, fov_closed_form):
        # The iteration in ONE library call (engine.retrieval_forward): the VMRs of the retrieved gases are set on the
        # device from the parameter vector (their profile IS sum_p mask_p x_p: LinearProfile_1D.profile), columns,
        # radiances + Jacobians, instrument bands and the pixels' closed-form FOV integral follow; one copy comes back.
        los, par_gas, par_w = _one_call_batch(scene, pixels, bayes_set, alts, with_fov)
        out, scene._fwd_buf = engine.retrieval_forward(coeffs, los, par_gas, par_w, bayes_set.param_vector(), scene.grid,
                                                       scene.bands_nm, scene.widths_nm, out_units=scene.out_units, g_lo=g_lo,
                                                       fov=scene._fov_fac if with_fov else None,
                                                       buf=getattr(scene, "_fwd_buf", None), ils=_ils(scene))
        if not with_fov:
            out = out[1::3]
        if shard is not None:
            out = _all_reduce_sum(out)
        return out[:, 0, :], out[:, 1:, :]
    los, alt = scene.los(alts)
    if bayes_set is None:
        rad = engine.limb_rays(coeffs, los)
        low = lowres(rad)
        both = low[:, None, :]
    else:
        par_gas, par_w = scene.profile_weights(bayes_set, alt)
        # radiances and derivatives in one buffer: one instrument-step launch and one copy to the host per iteration
        _, _, buf = engine.limb_rays_jacobian(coeffs, los, par_gas, par_w, joint=True, resident=True)
        n_par = len(par_gas)
        lo_all = lowres(buf)
        both = np.concatenate([lo_all[:n_los, None, :], lo_all[n_los:].reshape(n_los, n_par, -1)], axis=1)
    if shard is not None:
        both = _all_reduce_sum(both)     # the one exchange of a sharded iteration
    if alts_pix is not None:
        # group_observations: every quantity (radiance, each derivative) from its spline over the simulated ladder
        at = np.empty((len(alts_pix),) + both.shape[1:])
        for q in range(both.shape[1]):
            f = smm.make_radtran_spline(alts, np.ascontiguousarray(both[:, q, :]))
            for i, a in enumerate(alts_pix):
                at[i, q] = f(a)
        both = at
    low = both[:, 0, :]
    dlow = None if bayes_set is None else both[:, 1:, :]
    sims, derivs = [], []
    grid_lo = _Grid(scene.bands_nm)              # shared by the iteration's spectra (never modified)

    def spectrum_of(v):
        sp = Spectrum.__new__(Spectrum)
        sp.spectrum, sp.spectral_grid = v, grid_lo
        return sp

    # pixels with a field of view: the closed form for all of them in one pass -- the same elementwise operations on
    # [n_pix, 1 + n_par, n_bands] stacks, a rotation per pixel (it was 45 us of a 640 us configs[4] iteration)
    fov_all = None
    if fov_closed_form and pixels and all(pix.fov_half > 0 for pix in pixels):
        fov_all = smm.fov_closed_form(both[0::3], both[1::3], both[2::3], [pix.pixel_rot for pix in pixels])
    if arrays:
        if fov_all is None:
            _closed_form_fov(pixels, fov_closed_form, "simulate(arrays=True)")
            fov_all = both[1::3]
        return fov_all[:, 0, :], fov_all[:, 1:, :]
    for i, pix in enumerate(pixels):
        if pix.fov_half > 0 and fov_closed_form:
            # the closed form is linear in the three spectra: the pixel's radiances and all its derivatives at once
            # (FOV_integr_1D per spectrum, 8 per pixel, was a third of a configs[4] iteration's host time)
            fov = fov_all[i] if fov_all is not None else \
                smm.fov_closed_form(both[3 * i], both[3 * i + 1], both[3 * i + 2], pix.pixel_rot)   # [1 + n_par, n_bands]
            sims.append(spectrum_of(np.array(fov[0])))
            if dlow is not None:
                derivs.append([spectrum_of(np.array(fov[1 + p])) for p in range(dlow.shape[1])])
            continue
        three = [Spectrum(low[3 * i + q], scene.bands_nm) for q in range(3)]
        if pix.fov_half > 0:
            sims.append(smm.FOV_integr_1D(three, pix.pixel_rot, closed_form=fov_closed_form))
        else:
            sims.append(three[1])
        if dlow is not None:
            row = []
            for p in range(dlow.shape[1]):
                d3 = [Spectrum(dlow[3 * i + q, p], scene.bands_nm) for q in range(3)]
                row.append(smm.FOV_integr_1D(d3, pix.pixel_rot, closed_form=fov_closed_form) if pix.fov_half > 0 else d3[1])
            derivs.append(row)
    return sims, derivs


def _observed(pixels):
    """(obs, noise, masks) of the pixels, as lists; masks None when no pixel has one."""
    masks = None if all(pix.mask is None for pix in pixels) else [pix.mask for pix in pixels]
    return [pix.observation for pix in pixels], [pix.noise for pix in pixels], masks


class _Observations(object):
    """The observation side of a retrieval on arrays: the pixels' obs / noise / masks lists, their masked vectors obs_vec /
    noi_vec (smm.genvec), masktot (None: no pixel has a mask) and the inverse a-priori covariance Sa_inv of bayes_set --
    and what a loop does with an iteration's low [n_pix, n_bands] and dlow [n_pix, n_par, n_bands] against them: the same
    numbers in the same operations as the object path (genvec / build_jacobian concatenate and mask exactly these rows)."""

    def __init__(self, pixels, bayes_set):
        self.pixels, self.bayes_set = pixels, bayes_set
        self.obs, self.noise, self.masks = _observed(pixels)
        self.obs_vec, _, self.noi_vec = smm.genvec(self.obs, self.obs, self.noise, masks=self.masks)
        self.masktot = None if self.masks is None else np.concatenate([np.asarray(m, dtype=bool) for m in self.masks])
        self.Sa_inv = np.linalg.inv(np.asarray(bayes_set.VCM_apriori(), dtype=float))

    def chi(self, low):
        """(sim_vec, chi square over the parameters in use) of the simulated spectra (chicalc, :2949)."""
        sim_vec = low.reshape(-1) if self.masktot is None else low.reshape(-1)[self.masktot]
        return sim_vec, np.sum(((self.obs_vec - sim_vec) / self.noi_vec) ** 2) / (len(self.obs_vec) - self.bayes_set.n_used_par())

    def jacobian(self, dlow):
        """[n_obs, n_par]: build_jacobian's rows, masked."""
        jac = np.transpose(dlow, (1, 0, 2)).reshape(dlow.shape[1], -1)
        return (jac if self.masktot is None else jac[:, self.masktot]).T

    def finish(self, low, dlow, grid):
        """The end of a loop: bayes_set.jacobian and the parameters' stored derivatives (:2929, 2940) are the last
        iteration's; returns its spectra as objects on `grid` (a _Grid).  low None (max_it = 0: nothing was simulated): []."""
        if low is None:
            return []

        def wrap(v):
            sp = Spectrum.__new__(Spectrum)
            sp.spectrum, sp.spectral_grid = np.array(v), grid
            return sp

        self.bayes_set.jacobian = self.jacobian(dlow)
        for num in range(len(self.pixels)):
            for ip, par in enumerate(self.bayes_set.params()):
                par.store_deriv(wrap(dlow[num, ip]), num=num)
        return [wrap(v) for v in low]


def _array_loop(ob, forward, after_update, chi_threshold, max_it, lambda_LM, L1_reg, check_log=None):
    """The optimal-estimation loop on arrays, shared by the drivers: per iteration forward() -> (low [n_pix, n_bands], dlow
    [n_pix, n_par, n_bands]), chi square against the _Observations `ob`, the reference's stopping rule (:2963-2973), the
    Levenberg-Marquardt step (smm.inversion_algebra_arrays, :2977) and after_update(), which carries the new parameters to
    wherever the next forward() reads them.  Sets .history and .stop on ob.bayes_set; returns (chi, low, dlow) of the last
    iteration (None each for max_it = 0) for ob.finish."""
    bayes_set = ob.bayes_set
    bayes_set.history, bayes_set.stop = [], 'max_it'
    chi_old, chi, low, dlow = None, None, None, None
    for num_it in range(max_it):
        low, dlow = forward()
        for par in bayes_set.params():
            par.set_used()
        sim_vec, chi = ob.chi(low)
        bayes_set.history.append(chi)
        if check_log is not None:
            check_log.write('Iteration {:2d}: chi is {:8.3f}\n'.format(num_it, chi))
        why = smm.retrieval_converged(chi, chi_old, chi_threshold)
        if why:
            bayes_set.stop = why
            break
        chi_old = chi
        bayes_set.jacobian = ob.jacobian(dlow)
        smm.inversion_algebra_arrays(bayes_set.jacobian, ob.obs_vec, sim_vec, ob.noi_vec, bayes_set, lambda_LM=lambda_LM,
                                     L1_reg=L1_reg, Sa_inv=ob.Sa_inv)
        after_update()
    return chi, low, dlow


def inversion_fast_limb(scene, bayes_set, pixels, chi_threshold=0.01, max_it=10, lambda_LM=0.1, L1_reg=False,
                        solo_simulation=False, check_log=None, fov_closed_form=True, shard=None, refresh=False,
                        group_observations=False, alt_step_sims=50., alt_first_los=None):
    """The retrieval loop of spect_main_module.inversion_fast_limb (:2725-2987): Levenberg-Marquardt
    optimal estimation of the VMR-profile parameters in bayes_set from the pixels' observations.
    Returns (chi, obs, sims, bayes_set) like the reference, plus .history on bayes_set (chi per iteration)
    and .stop ('converged' | 'raised' | 'max_it').  shard / refresh: see simulate (every rank of a multi-GPU run
    calls this with its own spectral shard; all ranks hold the same chi square history and parameters)."""
    _refuse_instr(bayes_set, "inversion_fast_limb")
    _refuse_many_slots(scene, "inversion_fast_limb")
    pixels = sorted(pixels, key=lambda x: x.limb_tg_alt)                       # :2607
    group = (alt_step_sims, alt_first_los) if group_observations else None     # :2668-2670

    def into_gases():                                                          # :2624-2625, 2984-2985
        for name in bayes_set.sets.keys():
            scene.gas(name).add_clim(bayes_set.sets[name].profile())

    into_gases()
    obs, noise, masks = _observed(pixels)
    # The loop on arrays: when every pixel has the closed-form field of view (or none has one) an
    # iteration's spectra stay [n_pix, (n_par,) n_bands] arrays (_Observations) and become spectrum objects
    # once, when the loop ends; otherwise the objects of the reference's loop, iteration by iteration.
    with_fov = sum(pix.fov_half > 0 for pix in pixels)
    fast = not solo_simulation and ((with_fov == len(pixels) and fov_closed_form) or with_fov == 0)
    if fast:
        ob = _Observations(pixels, bayes_set)

        def finish(low, dlow):
            if low is not None:
                scene.los([a for pix in pixels for a in pix.los_alts()])   # the batch's VMRs = the final profiles (host copy too)
            return ob.finish(low, dlow, _Grid(scene.bands_nm))
    # Round 6: the whole iteration in ONE library call where it can be (engine.retrieval_step: forward model, chi square
    # and the Levenberg-Marquardt algebra -- the n_par x n_par systems in the library's host code -- on one process, the
    # whole grid, no observation grouping); what stays here is the reference's bookkeeping: the positivity rule of the
    # update, the stopping rule, the history.
    one_step = STEP_IN_ONE_CALL and fast and shard is None and group is None and _one_call_eligible(pixels, bayes_set, fov_closed_form)
    if fast and not one_step:
        def forward():
            return simulate(scene, pixels, bayes_set, fov_closed_form=fov_closed_form, shard=shard, refresh=refresh, arrays=True,
                            group=group)

        chi, low, dlow = _array_loop(ob, forward, into_gases, chi_threshold, max_it, lambda_LM, L1_reg, check_log=check_log)
        return chi, obs, finish(low, dlow), bayes_set
    bayes_set.history, bayes_set.stop = [], 'max_it'
    if one_step:
        n_pb = len(pixels) * len(scene.bands_nm)
        obs_all = np.concatenate([np.asarray(o.spectrum, float) for o in obs])
        noi_all = np.concatenate([np.asarray(nz.spectrum, float) for nz in noise])
        oe = engine.OeProblem(obs_all, noi_all, ob.masktot, ob.Sa_inv, bayes_set.apriori_vector(), lambda_LM)
        assert obs_all.size == n_pb
        alts_all = [a for pix in pixels for a in pix.los_alts()]
    # (a sunlit scene's coefficient rows do not stay fixed: the solar attenuation follows the VMRs, and the solar pass is
    # redone between the iterations -- the loop below, one engine.retrieval_step and one coefficient_stack() per iteration)
    if one_step and LOOP_IN_ONE_CALL and not refresh and max_it > 0 and not scene.solar_gases():
        # The loop in ONE library call (sr_retrieval_loop_dev): iterations, stopping rule and the updates with their
        # positivity rule run in the library; the objects' bookkeeping is replayed here from the vectors it returns.
        coeffs = scene.coefficient_stack(refresh=False)
        los_b, par_gas, par_w = _one_call_batch(scene, pixels, bayes_set, alts_all, with_fov)
        params = list(bayes_set.params())
        for par in params:
            par.set_used()
        both, hist, xh, why, S_x, AVK, scene._fwd_buf = engine.retrieval_loop(
            coeffs, los_b, par_gas, par_w, bayes_set.param_vector(), scene.grid, scene.bands_nm, scene.widths_nm, oe,
            [bool(par.constrain_positive) for par in params], bayes_set.n_used_par(), chi_threshold=chi_threshold, max_it=max_it,
            out_units=scene.out_units, fov=scene._fov_fac if with_fov else None, buf=getattr(scene, "_fwd_buf", None),
            ils=_ils(scene))
        for k in range(1, len(xh)):                                            # update_params / update_par, :616-624
            bayes_set.old_params.append(bayes_set.values())
            for par, v in zip(params, xh[k]):
                par.old_values.append(par.value)
                par.value = v
        if AVK is not None:
            bayes_set.store_avk(AVK)
            bayes_set.store_VCM(S_x)
        bayes_set.history = [float(c) for c in hist]
        if check_log is not None:
            for num_it, c in enumerate(bayes_set.history):
                check_log.write('Iteration {:2d}: chi is {:8.3f}\n'.format(num_it, c))
        into_gases()
        if why:
            bayes_set.stop = why
        return bayes_set.history[-1], obs, finish(both[:, 0, :], both[:, 1:, :]), bayes_set
    chi_old, chi, sims, low, dlow = None, None, [], None, None
    for num_it in range(max_it):
        if one_step:
            coeffs = scene.coefficient_stack(refresh=refresh)
            los_b, par_gas, par_w = _one_call_batch(scene, pixels, bayes_set, alts_all, with_fov)
            both, chi_sum, n_used, dx, S_x, AVK, scene._fwd_buf = engine.retrieval_step(
                coeffs, los_b, par_gas, par_w, bayes_set.param_vector(), scene.grid, scene.bands_nm, scene.widths_nm, oe,
                out_units=scene.out_units, fov=scene._fov_fac if with_fov else None, buf=getattr(scene, "_fwd_buf", None),
                ils=_ils(scene))
            low, dlow = both[:, 0, :], both[:, 1:, :]
            for par in bayes_set.params():
                par.set_used()
            chi = chi_sum / (n_used - bayes_set.n_used_par())                                              # chicalc, :2949
        else:
            sims, derivs = simulate(scene, pixels, bayes_set, fov_closed_form=fov_closed_form, shard=shard, refresh=refresh, group=group)
            if solo_simulation:
                return None
            for num, row in enumerate(derivs):
                for par, der in zip(bayes_set.params(), row):
                    par.store_deriv(der, num=num)                              # :2929, 2940
                    par.set_used()
            chi = smm.chicalc(obs, sims, noise, masks, bayes_set.n_used_par())  # :2949
        bayes_set.history.append(chi)
        if check_log is not None:
            check_log.write('Iteration {:2d}: chi is {:8.3f}\n'.format(num_it, chi))
        why = smm.retrieval_converged(chi, chi_old, chi_threshold)             # :2963-2973
        if why:
            bayes_set.stop = why
            break
        chi_old = chi
        if one_step:                                                           # inversion_algebra's results, :2977
            bayes_set.update_params(dx)
            bayes_set.store_avk(AVK)
            bayes_set.store_VCM(S_x)
        else:
            smm.inversion_algebra(obs, sims, noise, bayes_set, lambda_LM=lambda_LM, L1_reg=L1_reg, masks=masks)  # :2977
        into_gases()
    return chi, obs, (finish(low, dlow) if fast else sims), bayes_set


def _rows_in_bayes_order(fov_rows, n_prof, is_point, is_instr, instr, bands_nm0, is_opt=None):
    """[n_pix, 1 + n_prof (+ 1) (+ 2), n_bands] -- the radiance, the profile parameters in BayesSet order, the pointing
    row if any BayesSet parameter is the pointing's, d / d centre and d / d ln width if any is the instrument's -> [n_pix,
    1 + n_tot, n_bands] with every set's columns where the set stands (is_point, is_instr [n_tot]: whose each parameter
    is); the "instr" set's by the chain rule (BandCalibration.jacobian_rows)."""
    is_opt = np.zeros_like(is_instr) if is_opt is None else is_opt     # (the "optics" set's rows stand behind the pointing row)
    out = np.empty((fov_rows.shape[0], 1 + is_instr.size, fov_rows.shape[2]))
    out[:, 0] = fov_rows[:, 0]
    out[:, 1:][:, ~(is_instr | is_point | is_opt)] = fov_rows[:, 1:1 + n_prof]
    at = 1 + n_prof
    if is_point.any():
        out[:, 1:][:, is_point] = fov_rows[:, at:at + 1]
        at += 1
    if is_opt.any():
        n_opt = int(is_opt.sum())
        out[:, 1:][:, is_opt] = fov_rows[:, at:at + n_opt]
        at += n_opt
    if is_instr.any():
        out[:, 1:][:, is_instr] = instr.jacobian_rows(bands_nm0, fov_rows[:, at], fov_rows[:, at + 1])
    return out


def _state_into_gases(scene, bayes_set):
    """The BayesSet's profiles into the gases: add_clim for the VMR sets, tvib = tvib0 + offset for the Tvib sets; the
    "temp" set into the scene, temps = temps0 + offset (temps0: the temperatures at the first such call; the number
    densities and the LOS columns stay as they are, see TempProfile); the "instr" set into the scene's bands,
    bands_nm = bands_nm0 + shift + slope (bands_nm0 - mean), widths_nm = widths_nm0 exp(ln_width); the "optics" set
    (HazeOptics), projected into its domain first, into the solar gases' g.solar and scene.sun.surface_albedo."""
    names, tvib = [g.name for g in scene.gases], {}
    for name in bayes_set.order:
        st = bayes_set.sets[name]
        if name in names:
            scene.gas(name).add_clim(st.profile())
            continue
        if name == INSTR_SET:
            scene.bands_nm, scene.widths_nm = st.bands(scene.bands_nm0, scene.widths_nm0)
            continue
        if name == POINTING_SET:      # (the driver adds the offset to its lines of sight)
            continue
        if name == OPTICS_SET:        # projected into the domain, then into g.solar and the sun (solar_key sees both)
            st.project()
            for (kind, gas), v in zip(st.keys, st.values()):
                if kind == "surface_albedo":
                    scene.sun.surface_albedo = v
                else:
                    scene.gas(gas).solar[kind] = v
            continue
        if name == "temp":
            if getattr(scene, "temps0", None) is None:
                scene.temps0 = scene.temps.copy()
            scene.temps = scene.temps0 + st.profile()
            continue
        _, gas, level = name.split(":")
        g = scene.gas(gas)
        tv = tvib.setdefault(gas, g.tvib0.copy())
        tv[int(level)] = g.tvib0[int(level)] + st.profile()
    for gas, tv in tvib.items():
        scene.gas(gas).set_tvib(tv)


def _state_call(scene, w, coeffs, dcoeffs, los, bands, **kw):
    """The one mixed-state library call of an inversion_state iteration for the StateWeights `w`: on the spectra (bands
    False: (rad, jac)) or on the instrument's bands (True: the [.., 1 + n_par (+ ..), n_bands] rows).  Its receiver is the
    engine.LevelFactoredSet of the level gases when there are several, the one LevelGas's lf, or the engine function when
    there is none; the row parameters are named only with dcoeffs (a temperature set).  kw: the route's own keywords
    (pointing, fov, ils, instrument, out_units)."""
    route = "state_bands" if bands else "state_jacobian"
    state = dict(par_gas=w.par_gas, par_w_col=w.par_w_col)
    if dcoeffs is not None:
        state.update(dcoeffs=dcoeffs, par_w_temp=w.par_w_temp)
    if len(w.level_gases) > 1:
        lfs = engine.LevelFactoredSet([(g.lf, i, g.rows, g.tvib) for g, i in zip(w.level_gases, w.gases)])
        call, head = getattr(lfs, route), (w.par_lgas, w.par_level, w.par_w_lev)
    elif w.level_gas is not None:
        lg = w.level_gas
        call, head = getattr(lg.lf, route), (lg.rows, lg.tvib, w.par_level, w.par_w_lev)
        state["gas"] = w.gas
    else:
        call, head = getattr(engine, "limb_rays_" + route), ()
        names = dict(par_w_col="par_w", par_w_temp="par_t")     # (what the engine functions call the two weight blocks)
        state = {names.get(k, k): v for k, v in state.items()}
    if bands:
        head += (scene.grid, scene.bands_nm, scene.widths_nm)
    return call(coeffs, los, *head, **state, **kw)


def inversion_state(scene, bayes_set, pixels, chi_threshold=0.01, max_it=10, lambda_LM=0.1, L1_reg=False,
                    fov_closed_form=True, bands_in_kernel=False, solar_attenuation=False, diffuse_jacobian=False):
    """inversion_fast_limb's loop for a MIXED state vector: VMR-profile sets (named after a gas) together with the
    vibrational-temperature sets of one LevelGas or of several (TvibProfile; several: engine.LevelFactoredSet, the same one
    call per iteration with the level parameters of all of them) and the kinetic-temperature set (TempProfile; with it the
    coefficients and their temperature derivatives are recomputed per iteration, LimbScene.temperature_derivatives, and
    the same call takes the third kind too; after the loop the scene holds the final temperatures while a plain gas's
    cached coefficients are the last iteration's: coefficients(refresh=True) recomputes them).  Per iteration: the profiles into the gases, the
    coefficient stack (the LevelGas recombines its tables when its Tvib moved), ONE Jacobian call for all LOS of all pixels
    and both kinds of parameter (LevelFactored.state_jacobian), the instrument bands, the closed-form field of view,
    chi square, the stopping rule and the Levenberg-Marquardt step (smm.inversion_algebra_arrays).  Returns
    (chi, obs, sims, bayes_set) with .history, .stop, .jacobian and the stored averaging kernel and covariance, like
    inversion_fast_limb.  Every pixel has the closed-form field of view, or none has a field of view.
    bands_in_kernel=True: the Jacobian call, the instrument bands and the field of view of an iteration are ONE library call
    (LevelFactored.state_bands / engine.limb_rays_state_bands): the recursion kernel integrates the bands itself and no
    hi-res radiance or Jacobian is written.  The same numbers up to the order of the band sums (1e-12 relative).
    A set named "instr" (BandCalibration: band shift, its slope over the bands, ILS width) is retrieved with the profiles:
    per iteration its values go into scene.bands_nm / widths_nm, the two instrument rows of the band integrals come from
    the same fused call (instrument=True) or, on the other route, from engine.hires_to_lowres_instrument on the radiance
    the Jacobian call wrote, and the set's Jacobian columns follow by the chain rule (BandCalibration.jacobian_rows); they
    stand where the set stands in the BayesSet.  Without such a set nothing changes.
    A set named "pointing" (Pointing: one tangent-altitude offset [km] common to all pixels) is retrieved with them: per
    iteration the lines of sight are the pixels' los_alts() plus the current offset, the calls are made with pointing=True
    on both routes and the pointing row (through the field of view like the others) is the set's Jacobian column, where
    the set stands in the BayesSet; it can stand beside an "instr" set.  The crossed shells are held fixed within an
    iteration and rebuilt between iterations.  Without such a set nothing changes.
    solar_attenuation=True, on a scene with solar gases: the VMR columns of every iteration's Jacobian carry the derivative
    through the solar optical depth too (LimbScene.solar_attenuation_jacobian: the scene keeps its solar rows,
    keep_solar_rows), added to the hi-res Jacobian before the band step, or, with bands_in_kernel, as hi-res rows of its
    own through hires_to_lowres and the closed-form field of view (both linear) onto the fused call's band rows.  The
    term's Q pass is a four-gas call: more gas slots raise ValueError.  False, or a scene without a sun: nothing changes.
    diffuse_jacobian=True, on a scene with a Sun(multiple=True) and a solar gas: the VMR columns also carry the derivative
    through the diffuse rows' two-stream solve (LimbScene.diffuse_jacobian: the scene keeps the diffuse pass's inputs,
    keep_diffuse_state), added at the same two sites.  Independent of solar_attenuation: the full derivative of a sunlit
    multiple-scattering scene needs both flags.  The same four-gas Q pass, the same ValueError.  False, or a scene
    without such a sun: nothing changes.
    The temperature, vibrational-temperature, pointing and instrument columns have no such term here.
    A set named "optics" (HazeOptics: albedo and g of solar gases, the surface albedo) is retrieved with them: per
    iteration its projected values go into g.solar and scene.sun.surface_albedo (the solar pass is redone: solar_key sees
    them), and its columns are LimbScene.optics_jacobian's rows -- always the full derivative, whatever the two flags say
    -- added as hi-res rows before the band step or, with bands_in_kernel, as rows of their own through hires_to_lowres
    and the closed-form field of view; they stand where the set stands in the BayesSet.  The same four-gas limit and
    ValueError.  Without such a set no statement of an iteration changes."""
    pixels = sorted(pixels, key=lambda x: x.limb_tg_alt)
    with_fov = _closed_form_fov(pixels, fov_closed_form, "inversion_state")
    if getattr(scene, "thermal_scattering", None) is not None:
        if diffuse_jacobian:
            _refuse_thermal_scattering(scene, "inversion_state(diffuse_jacobian=True)")
        for name, st in bayes_set.sets.items():
            if isinstance(st, HazeOptics):
                _refuse_thermal_scattering(scene, "the HazeOptics set %r" % name)
            if isinstance(st, TempProfile):
                _refuse_thermal_scattering(scene, "the TempProfile set %r" % name)
    solar_att = bool(solar_attenuation) and bool(scene.solar_gases())
    if solar_att:
        if len(scene.gases) > engine.max_gases(folded=True):
            raise ValueError("inversion_state(solar_attenuation=True): a scene of %d gas slots; the term's Q pass "
                             "(engine.limb_rays_layer_jacobian) is a four-gas call" % len(scene.gases))
        scene.keep_solar_rows = True
    diffuse_jac = bool(diffuse_jacobian) and bool(scene.solar_gases()) and bool(getattr(scene.sun, "multiple", False))
    if diffuse_jac:
        if len(scene.gases) > engine.max_gases(folded=True):
            raise ValueError("inversion_state(diffuse_jacobian=True): a scene of %d gas slots; the term's Q pass "
                             "(engine.limb_rays_layer_jacobian) is a four-gas call" % len(scene.gases))
        scene.keep_diffuse_state = True
        scene._solar_key = None     # (a solar pass made before the flag kept nothing: the next one is made again)
    optics = bayes_set.sets.get(OPTICS_SET) if OPTICS_SET not in [g.name for g in scene.gases] else None
    is_opt = np.array([optics is not None and par.nameset == OPTICS_SET for par in bayes_set.params()], dtype=bool)
    if optics is not None:      # its columns are always the full derivative, whatever the two flags above say
        if not scene.solar_gases():
            raise ValueError("inversion_state: the retrieval set %r needs a scene with a sun and a solar gas" % OPTICS_SET)
        if len(scene.gases) > engine.max_gases(folded=True):
            raise ValueError("inversion_state with the retrieval set %r: a scene of %d gas slots; its Q pass "
                             "(engine.limb_rays_layer_jacobian) is a four-gas call" % (OPTICS_SET, len(scene.gases)))
        if getattr(scene.sun, "multiple", False):
            scene.keep_diffuse_state = scene.keep_mean_intensity = True
            scene._solar_key = None
    alts0 = [a for pix in pixels for a in pix.los_alts()]
    # the sets' names are checked before anything is changed
    with_temp = scene.state_weights(bayes_set, np.zeros(1), several_level_gases=True).par_w_temp.shape[0] > 0
    _state_into_gases(scene, bayes_set)
    ob = _Observations(pixels, bayes_set)
    lowres = lambda r: engine.hires_to_lowres(r, scene.grid, scene.bands_nm, scene.widths_nm, out_units=scene.out_units, ils=_ils(scene))
    rots = [pix.pixel_rot for pix in pixels]
    instr = bayes_set.sets.get(INSTR_SET) if INSTR_SET not in [g.name for g in scene.gases] else None
    is_instr = np.array([instr is not None and par.nameset == INSTR_SET for par in bayes_set.params()], dtype=bool)
    point = bayes_set.sets.get(POINTING_SET) if POINTING_SET not in [g.name for g in scene.gases] else None
    is_point = np.array([point is not None and par.nameset == POINTING_SET for par in bayes_set.params()], dtype=bool)
    point_kw = {} if point is None else dict(pointing=True)
    los_kw = {} if point is None else dict(path=True)
    n_los = len(alts0)
    # what the last forward() simulated on: its rays (a "pointing" set moves them) and its band centres (an "instr" set
    # moves those: the spectra carry the centres they were simulated on)
    alts, grid_sim = alts0, _Grid(scene.bands_nm)

    def forward():
        nonlocal alts, grid_sim
        coeffs, dcoeffs = (None if with_temp else scene.coefficient_stack()), None
        if point is not None:
            alts = [a + point.offset() for a in alts0]
        los, alt = scene.los(alts, **los_kw)
        if instr is not None:
            grid_sim = _Grid(scene.bands_nm.copy())
        w = scene.state_weights(bayes_set, alt, several_level_gases=True)
        if with_temp:    # coefficients at the current temperatures and their derivatives, then all three kinds at once
            coeffs, dcoeffs = (engine.gas_stack(c) for c in scene.temperature_derivatives())
        if bands_in_kernel:    # Jacobians, instrument bands and field of view in one call: [n_pix | n_los, 1 + n_par, n_bands]
            band_args = dict(out_units=scene.out_units, fov=engine.fov_factors(rots) if with_fov else None)
            if _ils(scene) is not None:
                band_args["ils"] = scene.ils
            if instr is not None:
                band_args["instrument"] = True
            both = _state_call(scene, w, coeffs, dcoeffs, los, True, **band_args, **point_kw)
            if (solar_att or diffuse_jac) and len(w.par_gas):    # the terms as hi-res rows of their own, through the band step and the field of view
                n_col = len(w.par_gas)
                term = scene.solar_attenuation_jacobian(los, alt, w, coeffs) if solar_att else None
                if diffuse_jac:
                    term = scene.diffuse_jacobian(los, alt, w, coeffs, term)
                extra = lowres(term.view(n_los * n_col, -1)).reshape(n_los, n_col, -1)
                if with_fov:
                    extra = smm.fov_closed_form(extra[0::3], extra[1::3], extra[2::3], rots)
                both = np.array(both)
                both[:, 1:1 + n_col] += extra
            n_par = both.shape[1] - 1 - (0 if instr is None else 2) - (0 if point is None else 1)
            fov = both if with_fov else both[1::3]
            fov = np.concatenate([fov[:, :1, :], fov[:, 1:1 + n_par, :][:, w.perm], fov[:, 1 + n_par:, :]], axis=1)
            if optics is not None:    # rows of their own through the band step and the field of view, as `extra` above
                n_opt = optics.n_par
                opt = lowres(scene.optics_jacobian(los, alt, optics.keys, coeffs).contiguous().view(n_los * n_opt, -1)).reshape(n_los, n_opt, -1)
                opt = smm.fov_closed_form(opt[0::3], opt[1::3], opt[2::3], rots) if with_fov else opt[1::3]
                at = 1 + n_par + (0 if point is None else 1)
                fov = np.concatenate([fov[:, :at, :], opt, fov[:, at:, :]], axis=1)
        else:
            if (instr is not None or optics is not None) and point is None and len(w.perm) == 0:    # the instrument (or optics) set alone: the radiances, no state Jacobian call
                rad, jac = engine.limb_rays(coeffs, los, resident=False), None
            else:
                rad, jac = _state_call(scene, w, coeffs, dcoeffs, los, False, **point_kw)
                if solar_att:
                    scene.solar_attenuation_jacobian(los, alt, w, coeffs, jac)
                if diffuse_jac:
                    scene.diffuse_jacobian(los, alt, w, coeffs, jac)
            n_rows = 0 if jac is None else jac.shape[1]
            n_par = n_rows - (0 if point is None else 1)               # (the pointing row stands behind the state's)
            order = np.concatenate([w.perm, np.arange(n_par, n_rows)]).astype(int)
            rows = [] if jac is None else [lowres(jac.contiguous().view(n_los * n_rows, -1)).reshape(n_los, n_rows, -1)[:, order]]
            if optics is not None:    # added as hi-res rows before the band step, behind the pointing row
                n_opt = optics.n_par
                rows.append(lowres(scene.optics_jacobian(los, alt, optics.keys, coeffs).contiguous().view(n_los * n_opt, -1)).reshape(n_los, n_opt, -1))
            if instr is None:
                both = np.concatenate([lowres(rad)[:, None, :]] + rows, axis=1)
            else:      # the instrument step once more on the radiance, with its two derivative rows (row 0: lowres(rad))
                three = engine.hires_to_lowres_instrument(rad, scene.grid, scene.bands_nm, scene.widths_nm, out_units=scene.out_units,
                                                          ils=_ils(scene))
                both = np.concatenate([three[0][:, None, :]] + rows + [three[1][:, None, :], three[2][:, None, :]], axis=1)
            fov = smm.fov_closed_form(both[0::3], both[1::3], both[2::3], rots) if with_fov else both[1::3]
        if instr is not None or point is not None or optics is not None:
            fov = _rows_in_bayes_order(fov, n_par, is_point, is_instr, instr, scene.bands_nm0, is_opt)
        return fov[:, 0, :], fov[:, 1:, :]

    chi, low, dlow = _array_loop(ob, forward, lambda: _state_into_gases(scene, bayes_set), chi_threshold, max_it, lambda_LM, L1_reg)
    if low is not None:
        scene.los(alts, **los_kw)                                  # the batch's VMRs = the final profiles
    return chi, ob.obs, ob.finish(low, dlow, grid_sim), bayes_set


class BoxPixel(LimbPixel):
    """A limb pixel in a scene whose composition depends on latitude: LimbPixel plus the latitude of its tangent point
    [deg] and the heading of its lines of sight there [deg east of north] (geometry.path_state_3d's frame).  The three
    rays of a pixel share both."""

    def __init__(self, limb_tg_alt, tangent_lat_deg, heading_deg=0.0, fov_half=0.0, pixel_rot=0.0, observation=None, noise=None,
                 mask=None):
        LimbPixel.__init__(self, limb_tg_alt, fov_half=fov_half, pixel_rot=pixel_rot, observation=observation, noise=noise, mask=mask)
        self.tangent_lat_deg, self.heading_deg = float(tangent_lat_deg), float(heading_deg)


class BoxBatch(object):
    """The LOS batch of a latitude-box scene (box_batch): L3 -- geometry.limb_los's dict of all pixels' three rays (low,
    centre, up; the coefficient rows are the altitude shells) with `seg_lat`, the latitude of every step --, par_gas
    [n_tot] and par_w [n_tot, n_pt], the weights of every parameter of the BayesSet at the sample points in BayesSet order,
    seg_box {set name: the box of every step} for the box sets, and touches [n_pix, n_tot]: parameter p has a non-zero
    weight at a sample point of one of the pixel's three rays (the complement is the reference's not_involved)."""

    def vmr(self, scene, bayes_set):
        """[n_gas, n_pt]: the VMRs at the sample points for the BayesSet's current values (a box set: geometry.box_vmr of
        its profile; a 1-D set: its profile, a gas without a set: its vmr, linear in altitude)."""
        from . import geometry
        zz, out = self.zz, []
        for g in scene.gases:
            st = bayes_set.sets.get(g.name)
            if isinstance(st, smm.LinearProfile_2D):
                out.append(geometry.box_vmr(self.L3, scene.z, st.profile(), self.seg_box[g.name]))
            else:
                v = np.asarray(g.vmr if st is None else st.profile(), float)
                out.append(np.interp(self.L3["alt"], zz, np.append(v, v[-1])))
        return np.array(out)

    def los(self, scene, bayes_set):
        """The engine.LimbLOS of the batch with vmr(scene, bayes_set); the caller closes it."""
        L3 = self.L3
        return engine.LimbLOS(L3["seg_off"], L3["seg_layer"], L3["pt_off"], L3["x"], L3["nd"], self.vmr(scene, bayes_set),
                              col_scale=[g.iso_ratio for g in scene.gases])


def box_batch(scene, bayes_set, pixels):
    """The BoxBatch of `pixels` (BoxPixel, taken in the order given) for the sets of bayes_set: smm.LinearProfile_2D sets
    named after gases of the scene (altitude nodes x latitude boxes) and 1-D profile sets of other gases."""
    from . import geometry
    names = [g.name for g in scene.gases]
    for name in bayes_set.order:
        if name not in names or not isinstance(bayes_set.sets[name], (smm.LinearProfile_2D, smm.LinearProfile_1D_new)):
            raise ValueError("retrieval set %r: inversion_boxes takes LinearProfile_2D and 1-D profile sets named after gases of "
                             "the scene" % (name,))
    alts = np.array([a for pix in pixels for a in pix.los_alts()])
    lat_t = np.repeat([pix.tangent_lat_deg for pix in pixels], 3)
    head = np.repeat([pix.heading_deg for pix in pixels], 3)
    L3 = dict(geometry.limb_los(scene.z, scene.nd, [g.vmr for g in scene.gases], alts, R=scene.R, n_sub=scene.n_sub))
    _, L3["seg_lat"] = geometry.path_state_3d(L3, alts, np.array([1.0, 0.0, 0.0]), head, lat_t, R=scene.R)
    B = BoxBatch()
    B.L3, B.alts, B.seg_box = L3, alts, {}
    B.zz = np.append(scene.z, scene.z[-1] + (scene.z[-1] - scene.z[-2]))
    par_gas, par_w = [], []
    for name in bayes_set.order:
        st = bayes_set.sets[name]
        par_gas += [names.index(name)] * len(st.set)
        if isinstance(st, smm.LinearProfile_2D):
            B.seg_box[name] = geometry.lat_box_of_segments(L3, st.lats)
            par_w.append(geometry.box_profile_weights(L3, scene.z, np.array([p.maskgrid.mask for p in st.set]), B.seg_box[name]))
        else:
            par_w.append(np.array([np.interp(L3["alt"], B.zz, np.append(p.maskgrid.mask, p.maskgrid.mask[-1])) for p in st.set]))
    B.par_gas, B.par_w = np.array(par_gas, np.int32), np.concatenate(par_w, axis=0)
    pt = np.asarray(L3["pt_off"])[np.asarray(L3["seg_off"])]            # first sample point of every ray
    B.touches = np.array([(B.par_w[:, pt[3 * i]:pt[3 * i + 3]] != 0).any(axis=1) for i in range(len(pixels))])
    return B


def inversion_boxes(scene, bayes_set, pixels, chi_threshold=0.01, max_it=10, lambda_LM=0.1, L1_reg=False, fov_closed_form=True):
    """The counterpart of the reference's inversion(..., g3D=True) (spect_main_module.py:2422-2595) for VMR sets of class
    smm.LinearProfile_2D, named after gases of the scene: a gas profile on altitude nodes x latitude boxes, retrieved
    from limb pixels (BoxPixel) whose lines of sight cross several boxes.  bayes_set may also hold 1-D profile sets of
    other gases.  T, P and the coefficient tables are the scene's 1-D ones (the rows are the altitude shells); only the
    composition varies with latitude.
    Per iteration: the box VMRs into the LOS batch of all pixels' three rays (geometry.box_vmr), ONE
    engine.limb_rays_state_bands call with the parameters' weights at the sample points (geometry.box_profile_weights),
    the field of view and ray_blocks=True -- a ray crosses two or three boxes and sees the nodes above its tangent
    altitude, so every ray is walked for its own parameters only --, chi square with n_tot parameters, the reference's
    stopping rule (smm.retrieval_converged) and smm.inversion_algebra_arrays.  A parameter that touches no ray of a
    pixel has exact-zero derivative rows there: the reference's not_involved (bayes_set.touches [n_pix, n_tot] says
    which; RetParam.not_involved is set for a parameter that touches no pixel at all).
    Returns (chi, obs, sims, bayes_set) with .history, .stop, .jacobian, .touches and the stored averaging kernel and
    covariance, as inversion_state.  Every pixel has the closed-form field of view, or none has a field of view.  After
    the loop a gas with a box set holds the final profiles in gas.vmr_boxes [n_box, n_lev]; its 1-D vmr is untouched."""
    pixels = sorted(pixels, key=lambda x: x.limb_tg_alt)
    with_fov = _closed_form_fov(pixels, fov_closed_form, "inversion_boxes")
    B = box_batch(scene, bayes_set, pixels)
    ob = _Observations(pixels, bayes_set)
    fov = engine.fov_factors([pix.pixel_rot for pix in pixels]) if with_fov else None
    band_args = dict(out_units=scene.out_units, fov=fov)
    if _ils(scene) is not None:
        band_args["ils"] = scene.ils
    bayes_set.touches = B.touches
    for ip, par in enumerate(bayes_set.params()):
        if B.touches[:, ip].any():
            par.set_involved()
        else:
            par.set_not_involved()

    def into_gases():
        for name in bayes_set.order:
            st = bayes_set.sets[name]
            if isinstance(st, smm.LinearProfile_2D):
                scene.gas(name).vmr_boxes = np.array(st.profile(), dtype=float)
            else:
                scene.gas(name).add_clim(st.profile())

    into_gases()
    los = B.los(scene, bayes_set)

    def forward():
        coeffs = scene.coefficient_stack()
        if bayes_set.history:      # (every iteration but the first, whose VMRs the batch was built with)
            los.set_vmr(B.vmr(scene, bayes_set))
        both = engine.limb_rays_state_bands(coeffs, los, scene.grid, scene.bands_nm, scene.widths_nm, par_gas=B.par_gas,
                                            par_w=B.par_w, ray_blocks=True, **band_args)
        rows = both if with_fov else both[1::3]
        return rows[:, 0, :], rows[:, 1:, :]

    try:
        chi, low, dlow = _array_loop(ob, forward, into_gases, chi_threshold, max_it, lambda_LM, L1_reg)
    finally:
        los.close()
    return chi, ob.obs, ob.finish(low, dlow, _Grid(scene.bands_nm)), bayes_set


def simulate_boxes(scene, bayes_set, pixels, fov_closed_form=True):
    """The band spectra [n_pix, n_bands] of `pixels` (BoxPixel, in the order given) for the BayesSet's current values: the
    forward model of inversion_boxes alone -- twin observations, finite differences."""
    with_fov = _closed_form_fov(pixels, fov_closed_form, "simulate_boxes")
    los = box_batch(scene, bayes_set, pixels).los(scene, bayes_set)
    try:
        rad = engine.limb_rays(scene.coefficient_stack(), los, resident=False)
        low = engine.hires_to_lowres(rad, scene.grid, scene.bands_nm, scene.widths_nm, out_units=scene.out_units, ils=_ils(scene))
    finally:
        los.close()
    if not with_fov:
        return low[1::3]
    return smm.fov_closed_form(low[0::3, None, :], low[1::3, None, :], low[2::3, None, :], [pix.pixel_rot for pix in pixels])[:, 0, :]


def lut_coefficients(scene, temp_step=5.0, pres_step_log=1.0, refresh=False, **_unused):
    """(abs, emi) of every gas at the scene's layer stack through look-up tables, the route of the reference's
    `inversion(..., useLUTs=True)` (spect_main_module.py:2447-2467 -> check_and_build_allluts; per LOS step
    LutSet.calculate, :997-1066): per gas and level the three G spectra on a rectangular (P, T) lattice that
    covers the atmosphere (temp_step [K], pres_step_log [ln hPa]: the reference's LUTopt keys) -- one
    sr_gcoeff_levels_dev call per gas (all levels from one walk of its lines), the table stays in HBM -- then per layer the bilinear interpolation and the
    population-weighted combine on the device (LutSet.combine_steps).  Tables are built once per scene."""
    import torch
    from . import spect_classes as spcl
    press, temps = scene.press, scene.temps
    Ps = np.exp(np.arange(np.floor(np.log(press.min())), np.log(press.max()) + pres_step_log, pres_step_log))
    Ts = np.arange(temp_step * np.floor(temps.min() / temp_step) - temp_step, temps.max() + 2 * temp_step, temp_step)
    PT = [[float(P), float(T)] for P in Ps for T in Ts]
    out = []
    for g in scene.gases + getattr(scene, "folded", []):
        _refuse_table_gas(g, "lut_coefficients (the look-up tables of G coefficients)")
    for g in scene.gases:
        ls = g.lineset
        n_lev = ls.level_energies.size
        if getattr(g, "luts", None) is None or refresh:
            g.luts = []
            # all levels of the lattice from one walk of the line list (sr_gcoeff_levels_dev: the multi-channel pass)
            g_all = ls.gcoeff_levels([pt[1] for pt in PT], [pt[0] for pt in PT])
            for lev in range(max(n_lev, 1)):
                lut = smm.LutSet(ls.mol, ls.iso, ls.mm, level=None, level_index=lev if n_lev else None)
                lut._append(g_all[lev], PT)
                g.luts.append(lut)
        q = np.atleast_1d(spcl.CalcPartitionSum(ls.mol, ls.iso, temps))
        ab = torch.zeros((len(temps), ls.n_grid), dtype=torch.float64, device="cuda")
        em = torch.zeros_like(ab)
        for lev, lut in enumerate(g.luts):
            if n_lev:
                tv = temps if g.tvib is None else np.asarray(g.tvib)[lev]
                pops = np.exp(-spcl.c2 * ls.level_energies[lev] / tv) / q           # smm:2073
            else:
                pops = 1.0 / q                                                       # smm:2054
            lut.combine_steps(press, temps, pops, ab, em)
        out.append((ab, em))
    return out


def inversion(scene, bayes_set, pixels, chi_threshold=0.01, max_it=10, lambda_LM=0.1, L1_reg=False, useLUTs=True,
              LUTopt=None, debugfile=None, fov_closed_form=True):
    """The reference's first retrieval driver, spect_main_module.inversion (:2422-2595; radtran_test_CO.py:189 calls
    it with useLUTs=True): pixel by pixel the three lines of sight of the FOV (low / centre / up), radiances and
    derivatives of every parameter involved, hires_to_lowres, FOV_integr_1D, then chi square over all pixels with
    n_tot parameters (:2562 -- the fast loop uses the parameters in use), the same stopping rule and
    inversion_algebra.  Coefficients through look-up tables (useLUTs, lut_coefficients) or directly.  Like the
    reference it returns None: the result is the state of bayes_set (.history, .stop are added)."""
    _refuse_instr(bayes_set, "inversion")
    _refuse_many_slots(scene, "inversion")
    LUTopt = dict(LUTopt or {})
    for name in bayes_set.sets.keys():                                                    # :2445-2446
        scene.gas(name).add_clim(bayes_set.sets[name].profile())
    coeffs = lut_coefficients(scene, **LUTopt) if useLUTs else scene.coefficients()
    obs, noise, masks = _observed(pixels)
    bayes_set.history, bayes_set.stop = [], 'max_it'
    sims = [None] * len(pixels)
    chi_old = None
    for num_it in range(max_it):
        if not useLUTs and scene.solar_gases():     # the solar attenuation follows the VMRs: the solar pass again (nothing else is rebuilt)
            coeffs = scene.coefficients()
        for num, pix in enumerate(pixels):                                                 # :2487
            los, alt = scene.los(pix.los_alts())                                           # low_LOS, LOS, up_LOS
            par_gas, par_w = scene.profile_weights(bayes_set, alt)
            rad, jac = engine.limb_rays_jacobian(coeffs, los, par_gas, par_w)
            low = engine.hires_to_lowres(rad, scene.grid, scene.bands_nm, scene.widths_nm, out_units=scene.out_units, ils=_ils(scene))
            dlow = engine.hires_to_lowres(jac.reshape(3 * len(par_gas), -1), scene.grid, scene.bands_nm, scene.widths_nm,
                                          out_units=scene.out_units, ils=_ils(scene)).reshape(3, len(par_gas), -1)
            three = [Spectrum(low[q], scene.bands_nm) for q in range(3)]
            sims[num] = smm.FOV_integr_1D(three, pix.pixel_rot, closed_form=fov_closed_form) if pix.fov_half > 0 else three[1]
            for p, par in enumerate(bayes_set.params()):
                if par.not_involved:                                                        # :2507-2509: zero derivative
                    par.store_deriv(Spectrum(np.zeros_like(low[0]), scene.bands_nm), num=num)
                    continue
                d3 = [Spectrum(dlow[q, p], scene.bands_nm) for q in range(3)]
                par.store_deriv(smm.FOV_integr_1D(d3, pix.pixel_rot, closed_form=fov_closed_form) if pix.fov_half > 0 else d3[1],
                                num=num)
                par.set_used()
        chi = smm.chicalc(obs, sims, noise, masks, bayes_set.n_tot)                        # :2562
        bayes_set.history.append(chi)
        why = smm.retrieval_converged(chi, chi_old, chi_threshold)                        # :2564-2570
        if why:
            bayes_set.stop = why
            return None
        chi_old = chi
        smm.inversion_algebra(obs, sims, noise, bayes_set, lambda_LM=lambda_LM, L1_reg=L1_reg, masks=masks)   # :2573
        if debugfile is not None:
            import pickle
            pickle.dump([num_it, [o.spectrum for o in obs], [s_.spectrum for s_ in sims], bayes_set.values()], debugfile)
        for name in bayes_set.sets.keys():                                                # :2581-2582
            scene.gas(name).add_clim(bayes_set.sets[name].profile())
    return None


def radtrans(scene, pixels, fov_closed_form=True, shard=None, group_observations=False, alt_step_sims=50., alt_first_los=None,
             track_levels=None, full_output=False):
    """Simulation only (spect_main_module.radtrans, :2990-3287): the FOV-integrated low-resolution spectra.
    group_observations / alt_step_sims / alt_first_los as in the reference's signature (:2990): simulate a ladder of
    tangent altitudes and spline to the pixels' lines of sight (simulate(group=...)).

    track_levels ({(gas.name, 'iso_<n>'): levels}, smm.track_all_levels(scene) for all of them; a level is an index or
    'lev_NN') or full_output=True: returns (sims, radtrans, single_rads) like the reference (:3287).  radtrans[tag] is
    the low-resolution spectrum of simulated line of sight tag = 'LOS%02d' (three per pixel in the pixels' order; the
    ladder's with group_observations), single_rads[(gas.name, 'iso_<n>')][tag] the part of it that gas emits and
    single_rads[(gas.name, 'iso_<n>', lev)][tag] the part a tracked level emits (engine.limb_rays_parts: each attenuated
    by all gases), without field-of-view integral, as in the reference.  The gases' spectra of a line of sight add up
    to its radtrans entry (the scene has no background), the levels' spectra of a gas to the gas's."""
    _refuse_many_slots(scene, "radtrans")
    group = (alt_step_sims, alt_first_los) if group_observations else None
    if track_levels is not None or full_output:
        return simulate(scene, pixels, None, fov_closed_form=fov_closed_form, shard=shard, group=group,
                        track_levels=track_levels, full_output=True)
    return simulate(scene, pixels, None, fov_closed_form=fov_closed_form, shard=shard, group=group)[0]
