"""Host-side engine objects over the C ABI: device-resident line sets, per-layer
coefficient spectra, limb radiances.  torch is used for device memory, streams
and (in distributed.py) the RCCL all-gather only.
"""
import collections
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import lib, check, dp, ip


def _d(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(dp)


def _i(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(ip)


_GRID_CACHE = []   # [(grid array, (w0, step, n))], the last few grids checked: a retrieval loop passes the same array in every iteration


def grid_params(grid):
    """(w0, step, n) of an equally spaced numpy-arange grid (spect_main_module.py:1267);
    raises if the grid is not exactly w0 + j*step.  The check walks the whole grid (1e5..2e6 points): the result is
    remembered for the array OBJECT it was made for (grids are not modified in place anywhere in this package)."""
    for g, res in _GRID_CACHE:
        # (identity alone says nothing about an array edited in place, ADVICE round 5: the remembered answer must still
        # describe the array's ends and length; an edit of interior points of a grid no caller makes goes unseen)
        if g is grid and g.size == res[2] and g[0] == res[0] and g[1] - g[0] == res[1] and g[-1] == res[0] + (res[2] - 1) * res[1]:
            return res
    arr = np.asarray(grid, dtype=np.float64)
    if arr.ndim != 1 or arr.size < 2:
        raise ValueError("spectral grid must be 1-D with at least 2 points")
    w0, step = float(arr[0]), float(arr[1] - arr[0])
    if not np.array_equal(arr, w0 + np.arange(arr.size) * step):
        raise ValueError("spectral grid is not an np.arange grid (w0 + j*step); the reference assumes "
                         "equal spacing (SpectralGrid.step, spect_classes.py:366)")
    res = (w0, step, arr.size)
    if isinstance(grid, np.ndarray):
        _GRID_CACHE[:] = [e for e in _GRID_CACHE if e[0] is not grid]
        _GRID_CACHE.append((grid, res))
        del _GRID_CACHE[:-8]
    return res


def set_device(index):
    check(lib.sr_set_device(int(index)), "sr_set_device")
    torch.cuda.set_device(int(index))


def device_info():
    name = C.create_string_buffer(256)
    cu = C.c_int(0)
    mem = C.c_double(0)
    check(lib.sr_device_info(name, 256, C.byref(cu), C.byref(mem)), "sr_device_info")
    rec, conf = C.c_int(0), C.c_int(0)
    check(lib.sr_recommended_hw_queues(C.byref(rec), C.byref(conf)), "sr_recommended_hw_queues")
    return dict(name=name.value.decode(), cu_count=cu.value, hbm_gib=mem.value, hw_queues=conf.value,
                hw_queues_recommended=rec.value)


def _stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class LineSet(object):
    """Device-resident line list of one iso-molecule bound to a spectral grid.

    lines: dict of arrays freq, a_coeff, e_lower, g_up, g_lo, air_broad, t_dep_broad
           [, lev_up, lev_lo] (SpectLine fields, spect_classes.py:50-51)
    level_energies: [] for the reference's 'all' set, else E_vib per level (cm^-1)
    """

    def __init__(self, lines, grid, mol, iso, mm, level_energies=()):
        self.w0, self.step, self.n_grid = grid_params(grid)
        self.mol, self.iso, self.mm = int(mol), int(iso), float(mm)
        self.level_energies = np.ascontiguousarray(level_energies, dtype=np.float64)
        keep = {}
        ld = _lib.LinesDesc()
        ld.n_lines = len(lines["freq"])
        for n in ("freq", "a_coeff", "e_lower", "g_up", "g_lo", "air_broad", "t_dep_broad"):
            keep[n], p = _d(lines[n])
            if keep[n].size != ld.n_lines:
                raise ValueError("line array %s has the wrong length" % n)
            setattr(ld, n, p)
        if self.level_energies.size:
            for n in ("lev_up", "lev_lo"):
                keep[n], p = _i(lines[n])
                setattr(ld, n, p)
        iso_d = _lib.IsoMolecDesc(self.mol, self.iso, self.mm, self.level_energies.size,
                                  self.level_energies.ctypes.data_as(dp))
        gd = _lib.GridDesc(self.w0, self.step, self.n_grid)
        h = C.c_void_p()
        kept = C.c_int64(0)
        check(lib.sr_lineset_create(C.byref(ld), C.byref(iso_d), C.byref(gd), C.byref(h), C.byref(kept)),
              "sr_lineset_create")
        self._h = h
        self.n_kept = kept.value
        self.n_lines_in = int(ld.n_lines)
        self._step_cache = None

    def close(self):
        if getattr(self, "_h", None) and lib is not None:
            lib.sr_lineset_destroy(self._h)
            self._h = None

    __del__ = close

    def _layers(self, temps, press, tvib, q_part):
        temps, tp = _d(temps)
        press, pp = _d(press)
        n = temps.size
        if press.size != n:
            raise ValueError("temps and press differ in length")
        keep = [temps, press]
        tvp = qp = None
        if tvib is not None:
            tvib, tvp = _d(tvib)
            if tvib.shape != (self.level_energies.size, n):
                raise ValueError("tvib must be [n_levels, n_layers]")
            keep.append(tvib)
        if q_part is not None:
            q_part, qp = _d(q_part)
            if q_part.size != n:
                raise ValueError("q_part must be [n_layers]")
            keep.append(q_part)
        return _lib.LayersDesc(n, tp, pp, tvp, qp), keep, n

    def abscoeff_layers(self, temps, press, tvib=None, q_part=None, g_lo=0, g_hi=None, out=None):
        """Per-layer abs/emi coefficient spectra on the GPU over grid shard [g_lo, g_hi).
        Returns two torch float64 CUDA tensors [n_layers, g_hi-g_lo] (HBM resident)."""
        g_hi = self.n_grid if g_hi is None else int(g_hi)
        desc, keep, n = self._layers(temps, press, tvib, q_part)
        npts = g_hi - int(g_lo)
        if npts <= 0:
            raise ValueError("empty shard")
        if out is None:
            ab = torch.empty((n, npts), dtype=torch.float64, device="cuda")
            em = torch.empty((n, npts), dtype=torch.float64, device="cuda")
        else:
            ab, em = out
            assert ab.shape == (n, npts) and em.shape == (n, npts) and ab.is_contiguous() and em.is_contiguous()
        check(lib.sr_abscoeff_layers_dev(self._h, C.byref(desc), int(g_lo), g_hi, C.c_void_p(ab.data_ptr()),
                                         C.c_void_p(em.data_ptr()), _stream_ptr()), "sr_abscoeff_layers_dev")
        return ab, em

    def set_strengths(self, s_ref, t_ref=296.0, iso_ab=1.0, q_ref=None):
        """HITRAN intensities of the lines, in the order given to the constructor (SpectLine.Strength:
        spect_classes.strengths_of): cm^-1 / (molecule cm^-2) at t_ref, abundance iso_ab included.  q_ref: Q(t_ref), None
        for CalcPartitionSum (sr_lineset_set_strengths).  They feed line_strengths(source="hitran") and
        abscoeff_layers_from_strengths."""
        s, sp = _d(s_ref)
        if s.ndim != 1 or s.size != self.n_lines_in:
            raise ValueError("s_ref must hold one intensity per input line (%d)" % self.n_lines_in)
        check(lib.sr_lineset_set_strengths(self._h, sp, int(s.size), float(t_ref), 0.0 if q_ref is None else float(q_ref),
                                           float(iso_ab)), "sr_lineset_set_strengths")

    def line_strengths(self, temps, tvib=None, q_part=None, source="einstein", iso_ab=1.0):
        """Strengths of every (layer, line) on the GPU (sr_line_strengths_dev): CUDA float64 (s_ab, s_em), each
        [n_layers, n_lines_in] in input order, 0 for the lines the filter dropped.  source "einstein":
        CalcStrength_from_Einstein times iso_ab; "hitran": CalcStrength_from_Strength from set_strengths' intensities
        (iso_ab unused).  tvib [n_levels, n_layers] or None (LTE)."""
        src = {"einstein": _lib.SR_STRENGTH_EINSTEIN, "hitran": _lib.SR_STRENGTH_HITRAN}.get(source)
        if src is None:
            raise ValueError("source must be 'einstein' or 'hitran'")
        t = np.atleast_1d(np.asarray(temps, dtype=np.float64))
        desc, keep, n = self._layers(t, np.zeros_like(t), tvib, q_part)
        s_ab = torch.empty((n, self.n_lines_in), dtype=torch.float64, device="cuda")
        s_em = torch.empty((n, self.n_lines_in), dtype=torch.float64, device="cuda")
        check(lib.sr_line_strengths_dev(self._h, C.byref(desc), src, float(iso_ab), C.c_void_p(s_ab.data_ptr()),
                                        C.c_void_p(s_em.data_ptr()), _stream_ptr()), "sr_line_strengths_dev")
        return s_ab, s_em

    def abscoeff_layers_from_strengths(self, temps, press, tvib=None, q_part=None, g_lo=0, g_hi=None, out=None):
        """abscoeff_layers with the lines weighted by their HITRAN strengths (set_strengths): s_ab / iso_ab and
        s_em / iso_ab of line_strengths(source="hitran") instead of the G coefficients
        (sr_abscoeff_layers_from_strengths_dev).  Same shapes, shards and modes as abscoeff_layers."""
        g_hi = self.n_grid if g_hi is None else int(g_hi)
        desc, keep, n = self._layers(temps, press, tvib, q_part)
        npts = g_hi - int(g_lo)
        if npts <= 0:
            raise ValueError("empty shard")
        if out is None:
            ab = torch.empty((n, npts), dtype=torch.float64, device="cuda")
            em = torch.empty((n, npts), dtype=torch.float64, device="cuda")
        else:
            ab, em = out
            assert ab.shape == (n, npts) and em.shape == (n, npts) and ab.is_contiguous() and em.is_contiguous()
        check(lib.sr_abscoeff_layers_from_strengths_dev(self._h, C.byref(desc), int(g_lo), g_hi, C.c_void_p(ab.data_ptr()),
                                                        C.c_void_p(em.data_ptr()), _stream_ptr()),
              "sr_abscoeff_layers_from_strengths_dev")
        return ab, em

    def limb_step(self, temps, press, los, tvib=None, q_part=None, g_lo=0, g_hi=None, out=None, rad=None, grid=None):
        """One forward-model step in ONE library call (sr_limb_step_dev): the coefficient spectra of this gas over
        [g_lo, g_hi) into `out` (as abscoeff_layers) and the radiances of the resident LOS batch `los` (LimbLOS, one
        gas) through them -- make_abscoeff_isomolec + radtran_fast per spectrum (spect_main_module.py:1979-1990, 2838).
        The layer descriptor is cached on the arrays' identity: a loop over the same atmosphere objects pays for
        neither conversions nor staging.  Returns (abs, emi, rad)."""
        g_hi = self.n_grid if g_hi is None else int(g_hi)
        key = (id(temps), id(press), id(tvib), id(q_part))
        c = self._step_cache
        if c is None or c[0] != key:
            desc, keep, n = self._layers(temps, press, tvib, q_part)
            c = (key, desc, keep, n)
            # cached only when the descriptor points into the caller's own arrays (contiguous float64: no copies were
            # made), so that values changed in place are seen; the arrays are referenced, their ids stay theirs
            given = [a for a in (temps, press, tvib, q_part) if a is not None]
            self._step_cache = c if all(any(k is a for k in keep) for a in given) else None
        _, desc, _, n = c
        npts = g_hi - int(g_lo)
        if npts <= 0:
            raise ValueError("empty shard")
        if out is None:
            out = (torch.empty((n, npts), dtype=torch.float64, device="cuda"), torch.empty((n, npts), dtype=torch.float64, device="cuda"))
        ab, em = out
        if rad is None:
            rad = torch.empty((los.n_rays, npts), dtype=torch.float64, device="cuda")
        assert ab.shape == (n, npts) and em.shape == (n, npts) and rad.shape == (los.n_rays, npts)
        assert ab.is_contiguous() and em.is_contiguous() and rad.is_contiguous()
        h = los.handle(n, grid)
        check(lib.sr_limb_step_dev(self._h, C.byref(desc), int(g_lo), g_hi, ab.data_ptr(), em.data_ptr(), h, rad.data_ptr(),
                                   _stream_ptr()), "sr_limb_step_dev")
        return ab, em, rad

    def set_bounds_temps(self, temps=None, linear_weights=False):
        """Place the Humlicek region boundaries of the next coefficient calls as at `temps` [n_layers] (None: at each
        call's own temperatures again): sr_lineset_set_bounds_temps.  For finite differences in T: c(T + dT) and c(T)
        then share their index-computed seams and the difference quotient is smooth (coefficients_dT).
        linear_weights: the line weights (G coefficients, normalisation) taken at `temps` and continued to the call's
        temperature to first order (sr_lineset_set_linear_weights): the quotient then has no curvature term from the
        Boltzmann factors and its step can be 0.05 K instead of 0.002 K (LevelFactored)."""
        if temps is None:
            check(lib.sr_lineset_set_bounds_temps(self._h, None, 0), "sr_lineset_set_bounds_temps")
            check(lib.sr_lineset_set_linear_weights(self._h, 0), "sr_lineset_set_linear_weights")
        else:
            t, tp = _d(temps)
            check(lib.sr_lineset_set_bounds_temps(self._h, tp, int(t.size)), "sr_lineset_set_bounds_temps")
            check(lib.sr_lineset_set_linear_weights(self._h, int(bool(linear_weights))), "sr_lineset_set_linear_weights")

    def set_line_shape(self, p_shift=None, self_broad=None):
        """Pressure shift of the line centres and self-broadening (sr_lineset_set_line_shape): p_shift and self_broad,
        cm^-1 / atm, one per input line in the constructor's order (SpectLine.P_shift, .Self_broad:
        spect_classes.line_shape_of).  Either may be None; both None restores the default, which is the reference's
        behaviour (centres at Freq, air broadening only).  Every later coefficient call on this line set places the
        shapes at Freq + p_shift P and takes lw = (296/T)^n (gamma_air (P - p_self) + gamma_self p_self), p_self from
        set_self_pressure."""
        ps = sb = None
        pp = sp = None
        n = 0
        if p_shift is not None:
            ps, pp = _d(p_shift)
            n = ps.size
        if self_broad is not None:
            sb, sp = _d(self_broad)
            n = sb.size
        for a in (ps, sb):
            if a is not None and (a.ndim != 1 or a.size != self.n_lines_in):
                raise ValueError("p_shift / self_broad must hold one value per input line (%d)" % self.n_lines_in)
        check(lib.sr_lineset_set_line_shape(self._h, pp, sp, int(n)), "sr_lineset_set_line_shape")

    def set_self_pressure(self, p_self=None):
        """Partial pressure of the gas itself, hPa per layer, for the following coefficient calls with that many layers
        (sr_lineset_set_self_pressure); None: 0 again.  It acts through set_line_shape's self_broad only."""
        if p_self is None:
            check(lib.sr_lineset_set_self_pressure(self._h, None, 0), "sr_lineset_set_self_pressure")
        else:
            p, pp = _d(np.atleast_1d(np.asarray(p_self, dtype=np.float64)))
            check(lib.sr_lineset_set_self_pressure(self._h, pp, int(p.size)), "sr_lineset_set_self_pressure")

    def gcoeff_layers(self, temps, press, level=0, g_lo=0, g_hi=None):
        """Per-ctype G-coefficient spectra of one level at every (P, T): CUDA float64
        [3, n_layers, g_hi-g_lo], ctype 0 sp_emission, 1 ind_emission, 2 absorption
        (sr_gcoeff_layers_dev = LutSet.add_PT / SpectralGcoeff.BuildCoeff)."""
        g_hi = self.n_grid if g_hi is None else int(g_hi)
        desc, keep, n = self._layers(temps, press, None, None)
        npts = g_hi - int(g_lo)
        if npts <= 0:
            raise ValueError("empty shard")
        g = torch.empty((3, n, npts), dtype=torch.float64, device="cuda")
        check(lib.sr_gcoeff_layers_dev(self._h, C.byref(desc), int(level), int(g_lo), g_hi,
                                       C.c_void_p(g.data_ptr()), _stream_ptr()), "sr_gcoeff_layers_dev")
        return g

    def gcoeff_levels(self, temps, press, g_lo=0, g_hi=None, out=None):
        """G-coefficient spectra of ALL levels at every (P, T): CUDA float64 [n_levels or 1, 3, n_rows, g_hi-g_lo], ctype
        0 sp_emission, 1 ind_emission, 2 absorption -- LookUpTable.make's inner loop over the levels
        (spect_main_module.py:759-772) in one call (sr_gcoeff_levels_dev: the multi-channel pass, every line once)."""
        g_hi = self.n_grid if g_hi is None else int(g_hi)
        desc, keep, n = self._layers(temps, press, None, None)
        npts = g_hi - int(g_lo)
        if npts <= 0:
            raise ValueError("empty shard")
        nl = max(int(self.level_energies.size), 1)
        if out is None:
            out = torch.empty((nl, 3, n, npts), dtype=torch.float64, device="cuda")
        assert out.shape == (nl, 3, n, npts) and out.is_contiguous() and out.dtype == torch.float64
        check(lib.sr_gcoeff_levels_dev(self._h, C.byref(desc), int(g_lo), g_hi, C.c_void_p(out.data_ptr()), _stream_ptr()),
              "sr_gcoeff_levels_dev")
        return out

    def glevel_pairs(self, temps, press, g_lo=0, g_hi=None, out=None):
        """Level-pair tables of the level-factored route (sr_glevel_pairs_dev): CUDA float64
        [n_levels or 1, 2, n_rows, g_hi-g_lo] with [L, 0] = Gabs_L - Gind_L and [L, 1] = Gsp_L at every (P, T) row --
        what pop_L multiplies in the reference's combine loop (spect_main_module.py:2073-2080).  No populations enter:
        the tables depend on (P, T) alone and serve every LOS step / SZA set that shares a row (glevel_combine)."""
        g_hi = self.n_grid if g_hi is None else int(g_hi)
        desc, keep, n = self._layers(temps, press, None, None)
        npts = g_hi - int(g_lo)
        if npts <= 0:
            raise ValueError("empty shard")
        nl = max(int(self.level_energies.size), 1)
        if out is None:
            out = torch.empty((nl, 2, n, npts), dtype=torch.float64, device="cuda")
        assert out.shape == (nl, 2, n, npts) and out.is_contiguous() and out.dtype == torch.float64
        check(lib.sr_glevel_pairs_dev(self._h, C.byref(desc), int(g_lo), g_hi, C.c_void_p(out.data_ptr()), _stream_ptr()),
              "sr_glevel_pairs_dev")
        return out

    def level_populations(self, temps, tvib=None, q_part=None, derivative=False):
        """pop [n_steps, n_levels or 1] = exp(-c2 E_L / Tvib_L) / Q(T) (spect_main_module.py:2049-2073; 1 / Q for the
        'all' set), tvib [n_levels, n_steps] or None (LTE: Tvib = T).  derivative=True: also d pop / d T with the
        vibrational temperatures held fixed when given (the definition of coefficients_dT), following T in LTE; Q'
        from the derivative of CalcPartitionSum's own interpolant unless q_part pins Q (then Q' = 0)."""
        from . import spect_classes as spcl
        T = np.ascontiguousarray(temps, dtype=np.float64)
        if q_part is not None:
            Q = np.asarray(q_part, float)
        else:   # on the distinct temperatures only (thousands of LOS steps share a few hundred)
            Tu, inv = np.unique(T, return_inverse=True)
            Q = np.atleast_1d(spcl.CalcPartitionSum(self.mol, self.iso, Tu))[inv]
        E = self.level_energies
        c2 = spcl.c2
        if E.size == 0:
            pop = (1.0 / Q)[:, None]
            boltz_dT = np.zeros_like(pop)
        else:
            tv = np.broadcast_to(T, (E.size, T.size)) if tvib is None else np.asarray(tvib, float)
            if tv.shape != (E.size, T.size):
                raise ValueError("tvib must be [n_levels, n_steps]")
            pop = (np.exp(-c2 * E[:, None] / tv) / Q[None, :]).T
            boltz_dT = (c2 * E[:, None] / tv ** 2).T if tvib is None else np.zeros((T.size, E.size))
        if not derivative:
            return np.ascontiguousarray(pop)
        dq = np.zeros_like(Q) if q_part is not None else np.atleast_1d(spcl.CalcPartitionSum_dT(self.mol, self.iso, T))
        dpop = pop * (boltz_dT - (dq / Q)[:, None])
        return np.ascontiguousarray(pop), np.ascontiguousarray(dpop)

    def level_populations_dtvib(self, temps, tvib, q_part=None):
        """d pop_L / d Tvib_L [n_steps, n_levels] = pop_L c2 E_L / Tvib_L^2 (spect_classes.level_populations_dtvib) with
        Q(T) supplied the way level_populations does.  ValueError for an iso-molecule without levels and in LTE
        (tvib None): the vibrational temperature is then not a variable."""
        from . import spect_classes as spcl
        if self.level_energies.size == 0:
            raise ValueError("the iso-molecule has no levels: no vibrational temperature to differentiate by")
        if tvib is None:
            raise ValueError("tvib is None (LTE): the vibrational temperature is not a variable")
        T = np.ascontiguousarray(temps, dtype=np.float64)
        if q_part is not None:
            Q = np.asarray(q_part, float)
        else:
            Tu, inv = np.unique(T, return_inverse=True)
            Q = np.atleast_1d(spcl.CalcPartitionSum(self.mol, self.iso, Tu))[inv]
        return spcl.level_populations_dtvib(self.level_energies, tvib, Q)

    def abscoeff_level(self, temps, press, level, tvib=None, q_part=None, g_lo=0, g_hi=None):
        """One level's share of abs / emi (track_levels, spect_main_module.py:2083-2087)."""
        g_hi = self.n_grid if g_hi is None else int(g_hi)
        desc, keep, n = self._layers(temps, press, tvib, q_part)
        npts = g_hi - int(g_lo)
        ab = torch.empty((n, npts), dtype=torch.float64, device="cuda")
        em = torch.empty((n, npts), dtype=torch.float64, device="cuda")
        check(lib.sr_abscoeff_level_dev(self._h, C.byref(desc), int(level), int(g_lo), g_hi,
                                        C.c_void_p(ab.data_ptr()), C.c_void_p(em.data_ptr()), _stream_ptr()),
              "sr_abscoeff_level_dev")
        return ab, em

    def abscoeff_layers_host(self, temps, press, tvib=None, q_part=None, g_lo=0, g_hi=None):
        """Same through the host-buffer entry point (numpy in, numpy out)."""
        g_hi = self.n_grid if g_hi is None else int(g_hi)
        desc, keep, n = self._layers(temps, press, tvib, q_part)
        ab = np.empty((n, g_hi - int(g_lo)))
        em = np.empty_like(ab)
        check(lib.sr_abscoeff_layers(self._h, C.byref(desc), int(g_lo), g_hi, ab.ctypes.data_as(dp),
                                     em.ctypes.data_as(dp)), "sr_abscoeff_layers")
        return ab, em

    def last_kernel_ms(self):
        """Kernel times (ms) of the last abscoeff_layers call: (prep, farfield|wings,
        near wings|cores, near zones|0, reserved); with overlap (default, far-field mode): (prep, whole
        coefficient op, 0, 0, 0).  See sr_last_kernel_ms."""
        ms = (C.c_float * 5)()
        check(lib.sr_last_kernel_ms(self._h, ms), "sr_last_kernel_ms")
        return tuple(ms)


    def last_level_tables_ms(self):
        """HIP-event times [ms] of the last multi-channel table build (glevel_pairs / gcoeff_levels): (tables, zones kernel,
        rest of the far passes, wings kernel); under set_overlap(0) the two kernels' stand-alone durations."""
        ms = (C.c_float * 4)()
        check(lib.sr_last_level_tables_ms(self._h, ms), "sr_last_level_tables_ms")
        return [float(v) for v in ms]

    def last_eval_counts(self):
        """Executed-work counters of the last abscoeff_layers call made under set_counting(1)
        (sr_last_eval_counts): dict name -> count."""
        c = (C.c_uint64 * 10)()
        check(lib.sr_last_eval_counts(self._h, c), "sr_last_eval_counts")
        names = ("farfield_expansions", "region1_evals", "window_end_expansions", "poly_point_levels",
                 "region2_evals", "region3_evals", "region4_evals", "multipole_line_sides", "box_pair_translations")
        return dict(zip(names, (int(v) for v in c)))


class AbsorberTable(object):
    """An absorber without lines -- a cross-section, collision-induced-absorption or extinction table -- resident on the
    device (sr_abs_table_create), put onto coefficient rows by layers().  The build's own definition; the
    reference has no counterpart.

    sets: a list of (T, v0, dv, values[, P]): a temperature (K), a regular wavenumber axis v0 + i dv (cm^-1) and the
          values on it, used as given, with an optional pressure label (hPa; all sets or none).  Or a dict of the arrays
          temp, v0, dv, off [n_sets + 1], values [, press].  One table is one spectral band: two sets of a pressure
          group may not share a temperature (bands of one species are summed with accumulate=True).
    """

    def __init__(self, sets):
        if isinstance(sets, dict):
            temp, v0, dv = (np.ascontiguousarray(sets[k], dtype=np.float64) for k in ("temp", "v0", "dv"))
            off = np.ascontiguousarray(sets["off"], dtype=np.int64)
            values = np.ascontiguousarray(sets["values"], dtype=np.float64)
            press = sets.get("press")
        else:
            sets = [tuple(s) for s in sets]
            if not sets or any(len(s) not in (4, 5) for s in sets):
                raise ValueError("a set is (T, v0, dv, values[, P])")
            if len({len(s) for s in sets}) != 1:
                raise ValueError("either all sets carry a pressure label or none does")
            temp = np.array([s[0] for s in sets], dtype=np.float64)
            v0 = np.array([s[1] for s in sets], dtype=np.float64)
            dv = np.array([s[2] for s in sets], dtype=np.float64)
            vals = [np.asarray(s[3], dtype=np.float64).ravel() for s in sets]
            off = np.concatenate([[0], np.cumsum([v.size for v in vals])]).astype(np.int64)
            values = np.ascontiguousarray(np.concatenate(vals))
            press = [s[4] for s in sets] if len(sets[0]) == 5 else None
        self.set_temp, self.set_v0, self.set_dv, self.set_off, self.values = temp, v0, dv, off, values
        self.set_press = None if press is None else np.ascontiguousarray(press, dtype=np.float64)
        self.n_sets = temp.size
        if not (v0.size == dv.size == self.n_sets and off.size == self.n_sets + 1 and values.size == (off[-1] if off.size else 0)):
            raise ValueError("the set arrays differ in length")
        if self.set_press is not None and (self.set_press.size != self.n_sets or not np.all(self.set_press > 0)):
            raise ValueError("pressure labels must be positive, one per set")
        self._groups()  # (refuses two sets of one group at one temperature)
        self._h = None  # made by the first layers(): plan() and the host layers above need no device

    def _handle(self):
        if self._h is None:
            h = C.c_void_p()
            check(lib.sr_abs_table_create(self.n_sets, self.set_temp.ctypes.data_as(dp), self.set_v0.ctypes.data_as(dp),
                                          self.set_dv.ctypes.data_as(dp), self.set_off.ctypes.data_as(C.POINTER(C.c_int64)),
                                          self.values.ctypes.data_as(dp), C.byref(h)), "sr_abs_table_create")
            self._h = h
        return self._h

    def close(self):
        if getattr(self, "_h", None) and lib is not None:
            lib.sr_abs_table_destroy(self._h)
            self._h = None

    __del__ = close

    def _groups(self):
        """[(P label or None, set indices in ascending temperature)], in ascending pressure."""
        if self.set_press is None:
            labels = [(None, np.arange(self.n_sets))]
        else:
            labels = [(p, np.nonzero(self.set_press == p)[0]) for p in np.unique(self.set_press)]
        out = []
        for p, idx in labels:
            idx = idx[np.argsort(self.set_temp[idx], kind="stable")]
            if np.any(np.diff(self.set_temp[idx]) == 0):
                raise ValueError("two sets of one pressure group share a temperature: one AbsorberTable is one band")
            out.append((p, idx))
        return out

    def plan(self, temps, press=None):
        """The rows' interpolation plan as plain arrays (set2 [n, 2] int32, w2 [n, 2], dw2 [n, 2]): which two sets a row
        at temps[r] (and press[r]) mixes, with which weights, and the weights' temperature derivatives.

        With pressure labels AND press, a row uses the group of sets whose label is nearest to its pressure in ln P (a
        tie goes to the lower pressure); otherwise all sets.  Inside the group, linear in T between the two bracketing
        sets, dw = -+1 / (T_hi - T_lo); outside the group's range the nearest set, w = (1, 0), dw = 0.  The larger
        weight is the quotient, the smaller one minus it (exact), so w_lo + w_hi == 1 and dw_lo + dw_hi == 0 exactly.
        ONE-SIDED at a set's temperature: a row exactly at T_k takes set k with weight 1 and the derivative of the
        interval ABOVE it (the right derivative of the piecewise-linear interpolant); at the group's hottest set there
        is no interval above, and the derivative is 0 as it is beyond it."""
        temps = np.atleast_1d(np.asarray(temps, dtype=np.float64))
        n = temps.size
        groups = self._groups()
        if press is not None and self.set_press is not None:
            lnp = np.log(np.broadcast_to(np.asarray(press, dtype=np.float64), (n,)))
        else:
            lnp = None
            if self.set_press is not None:  # no row pressure: every set, whatever its label
                groups = [(None, np.argsort(self.set_temp, kind="stable"))]
                if np.any(np.diff(self.set_temp[groups[0][1]]) == 0):
                    raise ValueError("sets of several pressure groups share temperatures: plan() needs press")
        set2, w2, dw2 = np.zeros((n, 2), np.int32), np.zeros((n, 2)), np.zeros((n, 2))
        for r in range(n):
            idx = groups[0][1]
            if lnp is not None:
                best = None
                for p, cand in groups:  # ascending pressure, strict <: a tie keeps the lower pressure
                    d = abs(lnp[r] - np.log(p))
                    if best is None or d < best:
                        best, idx = d, cand
            tk, T = self.set_temp[idx], temps[r]
            if T < tk[0] or idx.size == 1:
                set2[r], w2[r] = (idx[0], idx[0]), (1.0, 0.0)
            elif T >= tk[-1]:
                set2[r], w2[r] = (idx[-1], idx[-1]), (1.0, 0.0)
            else:
                k = int(np.searchsorted(tk, T, side="right")) - 1  # tk[k] <= T < tk[k + 1]
                span = tk[k + 1] - tk[k]
                if T - tk[k] >= tk[k + 1] - T:
                    hi = (T - tk[k]) / span
                    lo = 1.0 - hi
                else:
                    lo = (tk[k + 1] - T) / span
                    hi = 1.0 - lo
                set2[r], w2[r], dw2[r] = (idx[k], idx[k + 1]), (lo, hi), (-1.0 / span, 1.0 / span)
        return set2, w2, dw2

    def layers(self, temps, grid, press=None, scale=None, source=True, derivative=False, g_lo=0, g_hi=None, out=None,
               accumulate=False):
        """abs / emi (and with derivative=True their analytic d / dT, the scale held fixed) of the table on rows at temps
        over the grid shard [g_lo, g_hi): abs = scale (w_lo s_lo + w_hi s_hi) with the plan() of (temps, press) and the
        sets interpolated linearly to the grid, emi = abs B(nu, T) (source=False: 0).  accumulate=True adds to `out`.
        Returns (abs, emi) or ((abs, emi), (dabs, demi)): CUDA float64 [n_rows, g_hi - g_lo]."""
        w0, step, n_grid = grid_params(grid)
        g_hi = n_grid if g_hi is None else int(g_hi)
        npts = g_hi - int(g_lo)
        if npts <= 0:
            raise ValueError("empty shard")
        temps, tp = _d(np.atleast_1d(temps))
        n = temps.size
        set2, w2, dw2 = self.plan(temps, press)
        sc = scp = None
        if scale is not None:
            sc, scp = _d(np.broadcast_to(np.asarray(scale, dtype=np.float64), (n,)))
        n_out = 4 if derivative else 2
        if out is None:
            if accumulate:
                raise ValueError("accumulate=True adds to out=...")
            outs = [torch.empty((n, npts), dtype=torch.float64, device="cuda") for _ in range(n_out)]
        else:
            outs = list(out[0]) + list(out[1]) if derivative else list(out)
            for t in outs:
                assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.shape == (n, npts)
        ptr = lambda t: C.c_void_p(t.data_ptr())
        check(lib.sr_abs_table_layers_dev(self._handle(), n, tp, scp, set2.ctypes.data_as(ip), w2.ctypes.data_as(dp),
                                          dw2.ctypes.data_as(dp) if derivative else None, w0, step, int(g_lo), npts,
                                          int(bool(source)), int(bool(accumulate)), ptr(outs[0]), ptr(outs[1]),
                                          ptr(outs[2]) if derivative else None, ptr(outs[3]) if derivative else None,
                                          _stream_ptr()), "sr_abs_table_layers_dev")
        return ((outs[0], outs[1]), (outs[2], outs[3])) if derivative else (outs[0], outs[1])


def _cuda_f64(t):
    """A contiguous CUDA float64 tensor: what every device argument of the solar and diffuse calls is."""
    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()


def _chunk_lists(entry, name, d, n_k, n_tiles):
    """(tile_off [n_tiles + 1], chunks) of one of the two *_chunk_lists entries for the descriptor d."""
    n_chunks = (n_k + 3) // 4
    off, ch, n = np.zeros(n_tiles + 1, np.int32), np.zeros(max(n_tiles * n_chunks, 1), np.int32), C.c_int32(0)
    check(entry(C.byref(d), n_k, off.ctypes.data_as(ip), ch.ctypes.data_as(ip), C.byref(n)), name)
    return off, ch[:n.value].copy()


def _jac_target(out, par_slot, accumulate, n_rays, n_par, n_pts):
    """(out, the host array of par_slot, its pointer) of a Jacobian call that writes row par_slot[p] of out [n_rays,
    n_jac_rows, n_pts] for parameter p: None for out is a new [n_rays, n_par, n_pts] with row p."""
    slot, slot_p = _i(np.arange(n_par) if par_slot is None else par_slot)
    if slot.shape != (n_par,):
        raise ValueError("par_slot must be [n_par]")
    if out is None:
        if accumulate:
            raise ValueError("accumulate=True adds to out=...")
        if par_slot is not None:
            raise ValueError("par_slot places rows in out=...")
        out = torch.empty((n_rays, n_par, n_pts), dtype=torch.float64, device="cuda")
    elif not _cuda_f64(out) or out.dim() != 3 or out.shape[0] != n_rays or out.shape[2] != n_pts:
        raise ValueError("out must be a contiguous CUDA float64 [n_rays, n_jac_rows, n_pts]")
    return out, slot, slot_p


def _diffuse_state(A, V, ssa, asym, beam, sun, mu0, surface_albedo, night=False):
    """(sr_diffuse_desc, (n_gas, n_layers, n_pts), the host arrays it points to) of the state diffuse_source and
    diffuse_jacobian take, checked.  night=True (diffuse_thermal_source without a sun): beam and sun are None and not
    looked at, mu0 is 0."""
    lit = not night
    if not _cuda_f64(A) or A.dim() != 3 or (lit and (not (_cuda_f64(beam) and _cuda_f64(sun)) or beam.dim() != 2 or sun.dim() != 1)):
        raise ValueError("A, beam and sun must be contiguous CUDA float64 tensors ([n_gas, n_layers, n_pts], "
                         "[n_layers + 1, n_pts], [n_pts])")
    n_gas, n_layers, n_pts = (int(s) for s in A.shape)
    if n_gas == 0 or n_layers == 0 or n_pts == 0:
        raise ValueError("A must not be empty")
    va, vp = _d(np.asarray(V, dtype=np.float64))
    sa, sp = _d(np.broadcast_to(np.asarray(ssa, dtype=np.float64), (n_gas,)))
    ga, gp = _d(np.broadcast_to(np.asarray(asym, dtype=np.float64), (n_gas,)))
    if va.shape != (n_gas, n_layers):
        raise ValueError("V must be [n_gas, n_layers] = [%d, %d]" % (n_gas, n_layers))
    if lit and (beam.shape != (n_layers + 1, n_pts) or sun.shape[0] != n_pts):
        raise ValueError("beam must be [n_layers + 1, n_pts] and sun [n_pts] on A's %d grid points" % n_pts)
    d = _lib.DiffuseDesc()
    d.n_gas, d.n_layers, d.v, d.ssa, d.asym = n_gas, n_layers, vp, sp, gp
    d.mu0, d.surface_albedo = float(mu0) if lit else 0.0, float(surface_albedo)
    return d, (n_gas, n_layers, n_pts), (va, sa, ga)


def _solar_desc(U, w, src_row):
    """(sr_solar_desc, n_k, the arrays it points to) of U [n_rows, n_k] or [n_rows, n_gas, n_layers], w, src_row."""
    U = np.asarray(U, dtype=np.float64)
    if U.ndim not in (2, 3):
        raise ValueError("U must be [n_rows, n_k] or [n_rows, n_gas, n_layers]")
    u, up = _d(U.reshape(U.shape[0], -1))
    n_rows, n_k = u.shape
    wa, wp = _d(np.broadcast_to(np.asarray(w, dtype=np.float64), (n_rows,)))
    sa, sp = _i(np.arange(n_rows) if src_row is None else src_row)
    if sa.shape != (n_rows,):
        raise ValueError("src_row must be [n_rows]")
    d = _lib.SolarDesc()
    d.n_rows, d.u, d.w, d.src_row = n_rows, up, wp, sp
    return d, n_k, (u, wa, sa)


def set_solar_full_lists(on):
    """A check, not a mode of use: True makes solar_source (and solar_chunk_lists) list EVERY chunk of k on this thread
    until it is set back (sr_set_solar_full_lists) -- the chunks the lists skip only add exact zeros, so the result must
    come out bit for bit the same."""
    check(lib.sr_set_solar_full_lists(int(bool(on))), "sr_set_solar_full_lists")


def solar_chunk_lists(U, w):
    """(tile_off [n_tiles + 1], chunks) the solar-source kernel walks (sr_solar_chunk_lists, on the host: no GPU): per
    tile of 16 rows the chunks of four k in which any lit row (w != 0) of the tile has a non-zero column."""
    d, n_k, keep = _solar_desc(U, w, None)
    return _chunk_lists(lib.sr_solar_chunk_lists, "sr_solar_chunk_lists", d, n_k, (d.n_rows + 15) // 16)


def solar_source(A, U, w, sca, sun, src_row=None, out=None, accumulate=False, transmission=False):
    """The single-scattering solar source of coefficient rows (sr_solar_source_rows_dev; the build's own definition,
    DESIGN.md): sunlight, attenuated on its way in, scattered once into the line of sight, as emission rows

        tau[r] = sum_k U[r, k] A[k],   S[r] = w[r] sun exp(-tau[r]),   emi[r] (+)= sca[src_row[r]] S[r]

    A: the stacked absorption rows of the scene, CUDA [n_gas, n_layers, n_pts] (the first tensor of gas_stack) or
    [n_k, n_pts]; U: host [n_rows, n_gas, n_layers] or [n_rows, n_k], the slant columns towards the sun
    (geometry.solar_columns), >= 0, dense and mostly zeros; w: host [n_rows] = albedo x phase function / 4 pi, 0 for a row
    in shadow (exact 0 out, its optical depth not evaluated; under accumulate the row is left untouched); sca: CUDA
    [n_src, n_pts], the scatterer's own absorption rows; sun: CUDA [n_pts], the solar irradiance on the grid in units
    consistent with the emission rows; src_row [n_rows] (None: row r of sca).  out: CUDA [n_rows, n_pts], required with
    accumulate=True (thermal + solar).  transmission=True: also exp(-tau) itself [n_rows, n_pts] (1 for a row without
    columns, 0 in shadow and where tau >= 700).  One fused fp64 kernel; the same call gives the same bits.

    By default every Jacobian treats the rows as coefficients: the solar attenuation is HELD FIXED under d / d(VMR, T, Tvib)
    within one linearisation (as TempProfile holds columns and pressure fixed).  The derivative through tau for VMR
    parameters is solar_attenuation_jacobian (retrieval.inversion_state(solar_attenuation=True)), and through the diffuse
    rows made under this beam diffuse_jacobian (inversion_state(diffuse_jacobian=True)); for T and Tvib neither is
    built.  Returns emi, or (emi, trans)."""
    d, n_k, keep = _solar_desc(U, w, src_row)
    if not (_cuda_f64(A) and _cuda_f64(sca) and _cuda_f64(sun)) or A.dim() not in (2, 3) or sca.dim() != 2 or sun.dim() != 1:
        raise ValueError("A, sca and sun must be contiguous CUDA float64 tensors ([n_k or n_gas, n_layers, n_pts], [n_src, n_pts], [n_pts])")
    n_pts = A.shape[-1]
    if A.numel() != n_k * n_pts:
        raise ValueError("U has %d columns per row, A %d rows" % (n_k, A.numel() // max(n_pts, 1)))
    if sca.shape[1] != n_pts or sun.shape[0] != n_pts:
        raise ValueError("sca and sun must have A's %d grid points" % n_pts)
    if out is None:
        if accumulate:
            raise ValueError("accumulate=True adds to out=...")
        out = torch.empty((d.n_rows, n_pts), dtype=torch.float64, device="cuda")
    elif not _cuda_f64(out) or out.shape != (d.n_rows, n_pts):
        raise ValueError("out must be a contiguous CUDA float64 [n_rows, n_pts]")
    trans = torch.empty((d.n_rows, n_pts), dtype=torch.float64, device="cuda") if transmission else None
    check(lib.sr_solar_source_rows_dev(C.byref(d), C.c_void_p(A.data_ptr()), n_k, C.c_void_p(sca.data_ptr()), int(sca.shape[0]),
                                       C.c_void_p(sun.data_ptr()), n_pts, int(bool(accumulate)), C.c_void_p(out.data_ptr()),
                                       C.c_void_p(trans.data_ptr()) if transmission else None, _stream_ptr()),
          "sr_solar_source_rows_dev")
    return (out, trans) if transmission else out


def _diffuse_rules(out_gas, out, accumulate, asked, extra):
    """The rules among the arguments of a diffuse call's rows, which need no device: `extra` maps the entry's own row
    arguments to whether they are given, `asked`: J or F is."""
    if out_gas is None:
        if out is not None or accumulate or any(extra.values()):
            names = ["out", "accumulate"] + list(extra)
            raise ValueError("%s= and %s= belong to the rows of out_gas=" % ("=, ".join(names[:-1]), names[-1]))
        if not asked:
            raise ValueError("nothing asked for: out_gas=, mean_intensity=True or fluxes=True")
    elif out is None and accumulate:
        raise ValueError("accumulate=True adds to out=...")


def _diffuse_outputs(out_gas, out, accumulate, rows_shape, j_shape, f_shape, extra=None, rows="n_layers"):
    """The rows and outputs of a diffuse call: _diffuse_rules, then out checked against rows_shape (made where it is None
    and out_gas given; `rows` names its rows in the refusal) and J and F made where a shape is given.  Returns (out, J, F, result): the three as the C entry
    takes them, and what the call returns -- emi (if out_gas is given), then J, then F, as asked: one tensor or a tuple."""
    _diffuse_rules(out_gas, out, accumulate, j_shape is not None or f_shape is not None, extra or {})
    new = lambda shape: torch.empty(shape, dtype=torch.float64, device="cuda") if shape is not None else None
    if out_gas is not None:
        if out is None:
            out = new(rows_shape)
        elif not _cuda_f64(out) or out.shape != rows_shape:
            raise ValueError("out must be a contiguous CUDA float64 [%s, n_pts]" % rows)
    J, F = new(j_shape), new(f_shape)
    res = tuple(t for t in (out, J, F) if t is not None)
    return out, J, F, res[0] if len(res) == 1 else res


def diffuse_source(A, V, ssa, asym, beam, sun, mu0, surface_albedo=0.0, out_gas=None, out=None, accumulate=False,
                   mean_intensity=False, fluxes=False):
    """Multiple scattering of sunlight as emission rows (sr_diffuse_source_rows_dev; the build's own definition, DESIGN.md
    4.11b): per grid point a plane-parallel two-stream solve (Meador & Weaver's quadrature scheme) with delta scaling
    and a Lambertian lower boundary under the direct beam `beam`, and

        J[l] = sqrt3 (F+[l] + F-[l] + F+[l+1] + F-[l+1]) / (8 pi),   emi[l] (+)= ssa_G (1 - f_G) A[G, l] J[l]

    for the gas G = out_gas, f = max(asym, 0)^2.  The diffuse field holds light scattered once or more, so these rows
    are scattering orders two and above; order one stays solar_source's.

    A: the stacked absorption rows of the scene, CUDA [n_gas, n_layers, n_pts] (the first tensor of gas_stack); V: host
    [n_gas, n_layers] >= 0, the layers' vertical columns (geometry.vertical_columns); ssa [n_gas] in [0, 1] (0: an
    absorber) and asym [n_gas] in [-0.5, 1): host; beam: CUDA [n_layers + 1, n_pts], the direct beam's transmission at the
    layers' middle points and, last row, at the lower boundary (solar_source(..., transmission=True) with delta-scaled
    columns); sun: CUDA [n_pts]; mu0 = cos SZA; surface_albedo in [0, 1]: what lies below the lowest level.
    out_gas: the gas whose rows are made (None: no rows); out: CUDA [n_layers, n_pts], required with accumulate=True.
    mean_intensity=True: also J [n_layers, n_pts]; fluxes=True: also F [2, n_layers + 1, n_pts], F+ then F- at the
    interfaces.  One kernel, one writer per element; the same call gives the same bits.  By default every Jacobian
    treats the rows as coefficients; their derivative to VMR parameters is diffuse_jacobian
    (retrieval.inversion_state(diffuse_jacobian=True)), to T and Tvib it is not built.  Returns emi (if out_gas is given), then J, then F, as asked: one tensor or a tuple."""
    d, (n_gas, n_layers, n_pts), keep = _diffuse_state(A, V, ssa, asym, beam, sun, mu0, surface_albedo)
    out, J, F, res = _diffuse_outputs(out_gas, out, accumulate, (n_layers, n_pts), (n_layers, n_pts) if mean_intensity else None,
                                      (2, n_layers + 1, n_pts) if fluxes else None)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    check(lib.sr_diffuse_source_rows_dev(C.byref(d), ptr(A), ptr(beam), ptr(sun), n_pts, -1 if out_gas is None else int(out_gas),
                                         int(bool(accumulate)), ptr(out), ptr(J), ptr(F), _stream_ptr()),
          "sr_diffuse_source_rows_dev")
    return res


def diffuse_thermal_source(A, V, ssa, asym, temps, grid, t_surface=0.0, beam=None, sun=None, mu0=0.0, surface_albedo=0.0,
                           out_gas=None, out=None, accumulate=False, own_emission=False, mean_intensity=False, fluxes=False,
                           g_lo=0):
    """Thermal emission as a source of the two-stream diffuse field (sr_diffuse_thermal_rows_dev; the build's own
    definition): diffuse_source's solve with, per layer, the isotropic source 2 pi co B(nu, T_l) -- the
    layer emits (2 pi / sqrt3) B (1 - R - T) both ways, Kirchhoff's law; exactly 0 where the layer has no absorber -- and
    a Lambertian surface of emissivity 1 - surface_albedo at t_surface below (0: none).  beam, sun and mu0 as
    diffuse_source takes them add the sun's sources to the same solve (one walk of the layers for both); beam=None and
    sun=None is thermal emission alone, the night side: the call reads A only.

        own_emission=False:  emi[l] (+)= ssa_G (1 - f_G) A[G, l] J[l]
        own_emission=True:   emi[l] (+)= A[G, l] ((1 - ssa_G) B(nu, T_l) + ssa_G (1 - f_G) J[l])

    the second the scatterer's complete thermal row, in the place of a TableGas's emi = abs B (which emits as if all of
    the extinction were absorption).  For asym > 0 the forward peak's share of the line-of-sight source is left out, as
    in diffuse_source.  A, V, ssa, asym, surface_albedo, out_gas, out, accumulate, mean_intensity, fluxes and the result:
    as diffuse_source.  temps: host [n_layers] > 0; grid: the scene's spectral grid (grid_params), point j of A is grid
    point g_lo + j.  B is evaluated in the kernel as AbsorberTable.layers evaluates it.  Every Jacobian treats the rows
    as coefficients: their derivatives are not built."""
    # the rules among the arguments first, then the grid, then the tensors: what needs no device is refused without one
    if (beam is None) != (sun is None):
        raise ValueError("beam and sun: both (sunlight and thermal emission) or neither (thermal emission alone)")
    _diffuse_rules(out_gas, out, accumulate, mean_intensity or fluxes, {"own_emission": own_emission})
    w0, step, n_grid = grid_params(grid)
    ta, tp = _d(np.asarray(temps, dtype=np.float64))
    if ta.ndim != 1 or int(g_lo) < 0 or int(g_lo) >= n_grid:
        raise ValueError("temps must be [n_layers] and g_lo a point of the grid's %d" % n_grid)
    d, (n_gas, n_layers, n_pts), keep = _diffuse_state(A, V, ssa, asym, beam, sun, mu0, surface_albedo, night=beam is None)
    if ta.shape != (n_layers,):
        raise ValueError("temps must be [n_layers] = [%d]" % n_layers)
    if int(g_lo) + n_pts > n_grid:
        raise ValueError("the points g_lo .. g_lo + %d lie outside the grid's %d" % (n_pts, n_grid))
    th = _lib.DiffuseThermalDesc()
    th.temps, th.t_surface, th.w0, th.step, th.g_lo, th.own_emission = tp, float(t_surface), w0, step, int(g_lo), int(bool(own_emission))
    out, J, F, res = _diffuse_outputs(out_gas, out, accumulate, (n_layers, n_pts), (n_layers, n_pts) if mean_intensity else None,
                                      (2, n_layers + 1, n_pts) if fluxes else None)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    check(lib.sr_diffuse_thermal_rows_dev(C.byref(d), C.byref(th), ptr(A), ptr(beam), ptr(sun), n_pts,
                                          -1 if out_gas is None else int(out_gas), int(bool(accumulate)), ptr(out), ptr(J), ptr(F),
                                          _stream_ptr()), "sr_diffuse_thermal_rows_dev")
    return res


def diffuse_source_columns(A, V, ssa, asym, beams, sun, mu0s, col_w, row_layer, sca=None, src_row=None, surface_albedo=0.0,
                           out_gas=None, out=None, accumulate=False, mean_intensity=False, fluxes=False):
    """The diffuse field of diffuse_source for several columns of illumination over one atmosphere, and the emission rows
    of LOS steps that see it (sr_diffuse_source_columns_dev; the build's own definition): the steps of a
    3-D limb batch each have their own solar zenith angle.  Column c has mu0s[c] and beams[c]; J[c] and F[c] are exactly
    what diffuse_source defines for them (the atmosphere and its optics are shared, the columns independent), and

        emi[r] (+)= ssa_G (1 - f_G) sca[src_row[r]] sum_c col_w[r, c] J[c, row_layer[r]]

    for the gas G = out_gas.  A, V, ssa, asym, sun, surface_albedo: as diffuse_source takes them.  beams: CUDA [n_col,
    n_layers + 1, n_pts], n_col <= 8; mu0s: host [n_col]; col_w: host [n_rows, n_col] >= 0 (geometry.sza_columns: linear
    in mu0 between the columns); row_layer: host [n_rows], the layer of every row, in any order, a layer any number of
    times; sca: CUDA [n_src, n_pts], the scatterer's absorption on the rows' own places, and src_row [n_rows] (None: row
    r of sca); sca=None means A[out_gas] with src_row = row_layer.  out: CUDA [n_rows, n_pts], required with
    accumulate=True; a row whose weights are all zero is an exact 0 and, accumulating, keeps its bits.
    mean_intensity=True: also J [n_col, n_layers, n_pts]; fluxes=True: also F [n_col, 2, n_layers + 1, n_pts].  One kernel
    walks the layers once for all columns (the instance of the next column count of 1, 2, 4, 8); one writer per element;
    the same call gives the same bits, and a column's J and F do not depend on which columns share the call.  Every
    Jacobian treats these rows as coefficients.  Returns emi (if out_gas is given), then J, then F, as asked."""
    if not (_cuda_f64(A) and _cuda_f64(beams) and _cuda_f64(sun)) or A.dim() != 3 or beams.dim() != 3 or sun.dim() != 1:
        raise ValueError("A, beams and sun must be contiguous CUDA float64 tensors ([n_gas, n_layers, n_pts], "
                         "[n_col, n_layers + 1, n_pts], [n_pts])")
    if beams.shape[0] == 0:
        raise ValueError("beams must hold one column at the least")
    d, (n_gas, n_layers, n_pts), keep = _diffuse_state(A, V, ssa, asym, beams[0], sun, 0.0, surface_albedo)
    n_col = int(beams.shape[0])
    ma, mp = _d(np.asarray(mu0s, dtype=np.float64).reshape(-1))
    if ma.shape != (n_col,):
        raise ValueError("mu0s must be [n_col] = [%d], one per column of beams" % n_col)
    cd = _lib.DiffuseColumnsDesc()
    cd.n_col, cd.n_rows, cd.mu0 = n_col, 0, mp
    n_src = 0
    n_rows = 0
    if out_gas is not None:
        la, lp = _i(row_layer)
        if la.ndim != 1 or la.shape[0] == 0:
            raise ValueError("row_layer must be [n_rows], one row at the least")
        n_rows = la.shape[0]
        wa, wp = _d(np.asarray(col_w, dtype=np.float64))
        if wa.shape != (n_rows, n_col):
            raise ValueError("col_w must be [n_rows, n_col] = [%d, %d]" % (n_rows, n_col))
        if sca is None:
            if src_row is not None or not 0 <= int(out_gas) < n_gas:
                raise ValueError("sca=None takes A[out_gas] with src_row = row_layer")
            sca, src_row = A[int(out_gas)], la
        elif not _cuda_f64(sca) or sca.dim() != 2 or sca.shape[1] != n_pts:
            raise ValueError("sca must be a contiguous CUDA float64 [n_src, n_pts] on A's %d grid points" % n_pts)
        sa, sp = _i(np.arange(n_rows) if src_row is None else src_row)
        if sa.shape != (n_rows,):
            raise ValueError("src_row must be [n_rows]")
        n_src = int(sca.shape[0])
        cd.n_rows, cd.col_w, cd.row_layer, cd.src_row = n_rows, wp, lp, sp
        keep = keep + (la, wa, sa)
    out, J, F, res = _diffuse_outputs(out_gas, out, accumulate, (n_rows, n_pts), (n_col, n_layers, n_pts) if mean_intensity else None,
                                      (n_col, 2, n_layers + 1, n_pts) if fluxes else None, {"sca": sca is not None}, "n_rows")
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    check(lib.sr_diffuse_source_columns_dev(C.byref(d), C.byref(cd), ptr(A), ptr(beams), ptr(sun), n_pts, ptr(sca), n_src,
                                            -1 if out_gas is None else int(out_gas), int(bool(accumulate)), ptr(out), ptr(J), ptr(F),
                                            _stream_ptr()),
          "sr_diffuse_source_columns_dev")
    return res


SOLAR_JAC_RAYS = 8      # rays per block of sr_solar_jac_kernel (kSolarJacRays): where the ray-group edge of a call sits


def _solar_jac_desc(dU):
    """(sr_solar_jac_desc, n_k, the array it points to) of dU [n_par, n_rows, n_k] or [n_par, n_rows, n_gas, n_layers]."""
    dU = np.asarray(dU, dtype=np.float64)
    if dU.ndim not in (3, 4) or dU.shape[0] == 0 or dU.shape[1] == 0:
        raise ValueError("dU must be [n_par, n_rows, n_k] or [n_par, n_rows, n_gas, n_layers]")
    du, dup = _d(dU.reshape(dU.shape[0], dU.shape[1], -1))
    d = _lib.SolarJacDesc()
    d.n_par, d.n_rows, d.du = du.shape[0], du.shape[1], dup
    return d, du.shape[2], du


def solar_jacobian_chunk_lists(dU):
    """(tile_off [n_par n_tiles + 1], chunks) the solar-attenuation Jacobian kernel walks (sr_solar_jacobian_chunk_lists, on
    the host: no GPU): per parameter and tile of 16 rows the chunks of four k in which any row of the tile has a non-zero
    dU; the tiles of parameter p stand at p n_tiles .. (p + 1) n_tiles."""
    d, n_k, keep = _solar_jac_desc(dU)
    return _chunk_lists(lib.sr_solar_jacobian_chunk_lists, "sr_solar_jacobian_chunk_lists", d, n_k,
                        d.n_par * ((d.n_rows + 15) // 16))


def solar_attenuation_jacobian(A, dU, Q, out=None, par_slot=None, accumulate=False):
    """The solar attenuation in the Jacobians (sr_solar_jacobian_rows_dev; the build's own definition):
    the derivative of limb radiances to column parameters through the optical depth of solar_source's rows,

        dtau[p, r] = sum_k dU[p, r, k] A[k],   jac[ray, par_slot[p]] (+)= - sum_r Q[ray, r] dtau[p, r]

    A: the stacked absorption rows of the scene, CUDA [n_gas, n_layers, n_pts] or [n_k, n_pts], as solar_source takes
    them; dU: host [n_par, n_rows, n_gas, n_layers] or [n_par, n_rows, n_k] = d U / d x_p
    (geometry.solar_column_weights), any finite sign, dense and mostly zeros; Q: CUDA [n_rays, n_rows, n_pts], the
    derivative of the radiances to a factor 1 + eps_r on the solar part of row r's emission:
    limb_rays_layer_jacobian(coeffs, (zeros, solar rows), los).  out: CUDA [n_rays, n_jac_rows, n_pts], required with
    accumulate=True; par_slot [n_par]: the row of out of every parameter (None: row p, and out [n_rays, n_par, n_pts]);
    rows that are not named keep their bits.  One fused fp64 kernel; the same call gives the same bits.  Returns out."""
    d, n_k, keep = _solar_jac_desc(dU)
    if not (_cuda_f64(A) and _cuda_f64(Q)) or A.dim() not in (2, 3) or Q.dim() != 3:
        raise ValueError("A and Q must be contiguous CUDA float64 tensors ([n_k or n_gas, n_layers, n_pts], [n_rays, n_rows, n_pts])")
    n_pts = A.shape[-1]
    if A.numel() != n_k * n_pts:
        raise ValueError("dU has %d columns per row, A %d rows" % (n_k, A.numel() // max(n_pts, 1)))
    if Q.shape[0] == 0 or Q.shape[1] != d.n_rows or Q.shape[2] != n_pts:
        raise ValueError("Q must be [n_rays, %d, %d]: dU's rows and A's grid points" % (d.n_rows, n_pts))
    n_rays = int(Q.shape[0])
    out, slot, sp = _jac_target(out, par_slot, accumulate, n_rays, d.n_par, n_pts)
    check(lib.sr_solar_jacobian_rows_dev(C.byref(d), C.c_void_p(A.data_ptr()), n_k, C.c_void_p(Q.data_ptr()), n_rays, n_pts, sp,
                                         C.c_void_p(out.data_ptr()), int(out.shape[1]), int(bool(accumulate)), _stream_ptr()),
          "sr_solar_jacobian_rows_dev")
    return out


DIFFUSE_JAC_PARS = 4    # parameters per tile of sr_diffuse_tangent_kernel (kDiffuseJacPars): where a call's tile edge sits
DIFFUSE_JAC_RAYS = 8    # rays per thread of sr_diffuse_contract_kernel (kDiffuseJacRays)


def diffuse_jacobian(A, V, ssa, asym, beam, sun, mu0, dV, dlnbeam, Q, surface_albedo=0.0, out=None, par_slot=None,
                     accumulate=False, tangent=False):
    """The diffuse rows in the Jacobians (sr_diffuse_jacobian_rows_dev; the build's own definition): the
    derivative of limb radiances to column parameters through diffuse_source's two-stream solve,

        dJ[p, l] = the tangent of J[l] along d t_g[l] = dV[p, g, l] A[g, l], d ln D_l = dlnbeam[p, l],
                   d ln Ub_0 = dlnbeam[p, n_layers]
        jac[ray, par_slot[p]] (+)= sum_l Q[ray, l] dJ[p, l]

    of the function as built: the floor of co, g = 0 where nothing scatters and an empty layer have derivative 0.
    A, V, ssa, asym, beam, sun, mu0, surface_albedo: the state, as diffuse_source takes it.  dV: host [n_par, n_gas,
    n_layers] = d V / d x_p (geometry.vertical_column_weights), any finite sign, mostly zeros; dlnbeam: CUDA [n_par,
    n_layers + 1, n_pts] = d ln beam / d x_p, or None: the beam held fixed; Q: CUDA [n_rays, n_layers, n_pts] = d rad /
    d J_l: limb_rays_layer_jacobian(coeffs, (zeros, W), los) with W[g] = ssa_g (1 - f_g) A[g] for every solar gas, or None
    with tangent=True (dJ alone).  out: CUDA [n_rays, n_jac_rows, n_pts], required with accumulate=True; par_slot [n_par]:
    the row of out of every parameter (None: row p, and out [n_rays, n_par, n_pts]); rows that are not named keep their
    bits.  tangent=True: also dJ [n_par, n_layers, n_pts], the counterpart of diffuse_source(mean_intensity=True).  Two
    fp64 kernels, one writer per element; the same call gives the same bits.  Returns out, (out, dJ), or dJ (Q None)."""
    d, (n_gas, n_layers, n_pts), keep = _diffuse_state(A, V, ssa, asym, beam, sun, mu0, surface_albedo)
    dva, dvp = _d(np.asarray(dV, dtype=np.float64))
    if dva.ndim != 3 or dva.shape[0] == 0 or dva.shape[1:] != (n_gas, n_layers):
        raise ValueError("dV must be [n_par, n_gas, n_layers] = [n_par, %d, %d]" % (n_gas, n_layers))
    n_par = int(dva.shape[0])
    if dlnbeam is not None and (not _cuda_f64(dlnbeam) or dlnbeam.shape != (n_par, n_layers + 1, n_pts)):
        raise ValueError("dlnbeam must be a contiguous CUDA float64 [n_par, n_layers + 1, n_pts] or None")
    slot_p = None
    if Q is None:
        if not tangent:
            raise ValueError("nothing asked for: Q=... or tangent=True")
        if out is not None or par_slot is not None or accumulate:
            raise ValueError("out=, par_slot= and accumulate= belong to the product with Q=")
        n_rays = 0
    else:
        if not _cuda_f64(Q) or Q.dim() != 3 or Q.shape[0] == 0 or Q.shape[1] != n_layers or Q.shape[2] != n_pts:
            raise ValueError("Q must be a contiguous CUDA float64 [n_rays, %d, %d]: A's layers and grid points" % (n_layers, n_pts))
        n_rays = int(Q.shape[0])
        out, slot, slot_p = _jac_target(out, par_slot, accumulate, n_rays, n_par, n_pts)
    dJ = torch.empty((n_par, n_layers, n_pts), dtype=torch.float64, device="cuda") if tangent else None
    jd = _lib.DiffuseJacDesc()
    jd.n_par, jd.dv = n_par, dvp
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    check(lib.sr_diffuse_jacobian_rows_dev(C.byref(d), C.byref(jd), ptr(A), ptr(beam), ptr(sun), ptr(dlnbeam), ptr(Q), n_rays, n_pts,
                                           slot_p, ptr(out), int(out.shape[1]) if out is not None else 0, int(bool(accumulate)),
                                           ptr(dJ), _stream_ptr()), "sr_diffuse_jacobian_rows_dev")
    res = tuple(t for t in (out, dJ) if t is not None)
    return res[0] if len(res) == 1 else res


def diffuse_optics_jacobian(A, V, ssa, asym, beam, sun, mu0, dssa, dasym, dalbedo, dlnbeam, Q, surface_albedo=0.0, out=None,
                            par_slot=None, accumulate=False, tangent=False):
    """The diffuse rows along a direction in the haze optics (sr_diffuse_optics_jacobian_rows_dev; the build's own
    definition): the derivative of limb radiances to ssa, asym and the surface albedo through
    diffuse_source's two-stream solve,

        dJ[p, l] = the tangent of J[l] along d ssa_g = dssa[p, g], d asym_g = dasym[p, g], d surface_albedo = dalbedo[p],
                   d ln D_l = dlnbeam[p, l], d ln Ub_0 = dlnbeam[p, n_layers] (the beam's part of the boundary term)
        jac[ray, par_slot[p]] (+)= sum_l Q[ray, l] dJ[p, l]

    of the function as built (diffuse_jacobian's three rules; f = max(asym, 0)^2 has derivative 0 for asym <= 0).  A, V,
    ssa, asym, beam, sun, mu0, surface_albedo: the state, as diffuse_source takes it.  dssa, dasym: host [n_par, n_gas],
    dalbedo: host [n_par]; any finite sign; any of the three may be None (zeros), not all.  dlnbeam, Q, out, par_slot,
    accumulate, tangent: as diffuse_jacobian takes them.  No division by the albedo: 0 is an ordinary state.  Two fp64
    kernels, one writer per element; the same call gives the same bits.  Returns out, (out, dJ), or dJ (Q None)."""
    # (what needs no tensor is refused first, then the state is looked at)
    given = [np.asarray(x, dtype=np.float64) for x in (dssa, dasym, dalbedo) if x is not None]
    if not given:
        raise ValueError("nothing to differentiate along: dssa=, dasym= or dalbedo=")
    dims = [np.ndim(x) for x in (dssa, dasym) if x is not None] + ([np.ndim(dalbedo) + 1] if dalbedo is not None else [])
    if any(k != 2 for k in dims) or len({int(x.shape[0]) for x in given}) != 1 or given[0].shape[0] == 0:
        raise ValueError("dssa and dasym must be [n_par, n_gas] and dalbedo [n_par], one n_par >= 1 for all")
    n_par = int(given[0].shape[0])
    if Q is None and not tangent:
        raise ValueError("nothing asked for: Q=... or tangent=True")
    if Q is None and (out is not None or par_slot is not None or accumulate):
        raise ValueError("out=, par_slot= and accumulate= belong to the product with Q=")
    d, (n_gas, n_layers, n_pts), keep = _diffuse_state(A, V, ssa, asym, beam, sun, mu0, surface_albedo)
    od = _lib.DiffuseOpticsDesc()
    od.n_par = n_par
    held = []
    for name, x, shape in (("dssa", dssa, (n_par, n_gas)), ("dasym", dasym, (n_par, n_gas)), ("dalb", dalbedo, (n_par,))):
        if x is None:
            continue
        xa, xp = _d(np.asarray(x, dtype=np.float64))
        if xa.shape != shape:
            raise ValueError("dssa and dasym must be [n_par, n_gas] = [%d, %d] and dalbedo [%d]" % (n_par, n_gas, n_par))
        held.append(xa)
        setattr(od, name, xp)
    if dlnbeam is not None and (not _cuda_f64(dlnbeam) or dlnbeam.shape != (n_par, n_layers + 1, n_pts)):
        raise ValueError("dlnbeam must be a contiguous CUDA float64 [n_par, n_layers + 1, n_pts] or None")
    slot_p = None
    if Q is None:
        n_rays = 0
    else:
        if not _cuda_f64(Q) or Q.dim() != 3 or Q.shape[0] == 0 or Q.shape[1] != n_layers or Q.shape[2] != n_pts:
            raise ValueError("Q must be a contiguous CUDA float64 [n_rays, %d, %d]: A's layers and grid points" % (n_layers, n_pts))
        n_rays = int(Q.shape[0])
        out, slot, slot_p = _jac_target(out, par_slot, accumulate, n_rays, n_par, n_pts)
    dJ = torch.empty((n_par, n_layers, n_pts), dtype=torch.float64, device="cuda") if tangent else None
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    check(lib.sr_diffuse_optics_jacobian_rows_dev(C.byref(d), C.byref(od), ptr(A), ptr(beam), ptr(sun), ptr(dlnbeam), ptr(Q), n_rays,
                                                  n_pts, slot_p, ptr(out), int(out.shape[1]) if out is not None else 0,
                                                  int(bool(accumulate)), ptr(dJ), _stream_ptr()),
          "sr_diffuse_optics_jacobian_rows_dev")
    res = tuple(t for t in (out, dJ) if t is not None)
    return res[0] if len(res) == 1 else res


def lut_interp(table, idx4, wgt4, pops=None, out=None):
    """LutSet.calculate for n_steps LOS steps on a G table resident in HBM (sr_lut_interp_dev).
    table: CUDA [3, n_PT, n_grid]; idx4 [n_steps, 4] rows, wgt4 [n_steps, 4] = (wP1, wP2, wT1, wT2).
    pops None: returns the interpolated set [3, n_steps, n_grid]; else accumulates the population-weighted
    combine into out = (abs, emi), CUDA [n_steps, n_grid]."""
    assert table.is_cuda and table.dtype == torch.float64 and table.is_contiguous() and table.dim() == 3
    idx4, ipp = _i(np.asarray(idx4).reshape(-1, 4))
    wgt4, wp = _d(np.asarray(wgt4).reshape(-1, 4))
    n_steps, n_pt, n_pts = idx4.shape[0], table.shape[1], table.shape[2]
    if pops is None:
        g = torch.empty((3, n_steps, n_pts), dtype=torch.float64, device="cuda")
        check(lib.sr_lut_interp_dev(C.c_void_p(table.data_ptr()), n_pt, n_pts, n_steps, ipp, wp, None, 0,
                                    C.c_void_p(g.data_ptr()), None, _stream_ptr()), "sr_lut_interp_dev")
        return g
    pops, pp = _d(pops)
    ab, em = out
    for t in (ab, em):
        assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.shape == (n_steps, n_pts)
    check(lib.sr_lut_interp_dev(C.c_void_p(table.data_ptr()), n_pt, n_pts, n_steps, ipp, wp, pp, 1,
                                C.c_void_p(ab.data_ptr()), C.c_void_p(em.data_ptr()), _stream_ptr()),
          "sr_lut_interp_dev")
    return ab, em


def glevel_combine(tab, step_row, pop, tab_dT=None, dpop=None, dT=None, out=None):
    """The combine loop of the level-factored route for all LOS steps at once (sr_glevel_combine_dev):
    abs[s] = sum_L pop[s, L] tab[L, 0, row[s]], emi[s] = sum_L pop[s, L] tab[L, 1, row[s]] -- one pass over the pair
    tables (LineSet.glevel_pairs), the steps of a (P, T) row taken together.  With tab_dT (the tables at T + dT, region
    boundaries frozen at T), dpop [n_steps, n_levels] and dT also d abs / d T and d emi / d T of every step: population
    part analytic, d G / d T by difference.  Returns (abs, emi) or ((abs, emi), (dabs, demi)), CUDA [n_steps, n_pts]."""
    assert tab.is_cuda and tab.dtype == torch.float64 and tab.is_contiguous() and tab.dim() == 4 and tab.shape[1] == 2
    nl, _, n_rows, n_pts = tab.shape
    step_row, sp = _i(step_row)
    pop, pp = _d(pop)
    n_steps = step_row.size
    if pop.shape != (n_steps, nl):
        raise ValueError("pop must be [n_steps, n_levels]")
    want_dT = tab_dT is not None
    if want_dT:
        assert tab_dT.shape == tab.shape and tab_dT.is_contiguous() and tab_dT.dtype == torch.float64
        dpop, dpp = _d(dpop)
        if dpop.shape != pop.shape or not dT:
            raise ValueError("the temperature derivative needs dpop [n_steps, n_levels] and dT")
    else:
        dpp = None
    n_out = 4 if want_dT else 2
    if out is None:
        out = [torch.empty((n_steps, n_pts), dtype=torch.float64, device="cuda") for _ in range(n_out)]
    for t in out:
        assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.shape == (n_steps, n_pts)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    check(lib.sr_glevel_combine_dev(ptr(tab), ptr(tab_dT) if want_dT else None, nl, n_rows, n_pts, n_steps, sp, pp, dpp,
                                    (1.0 / dT) if want_dT else 0.0, ptr(out[0]), ptr(out[1]),
                                    ptr(out[2]) if want_dT else None, ptr(out[3]) if want_dT else None, _stream_ptr()),
          "sr_glevel_combine_dev")
    return ((out[0], out[1]), (out[2], out[3])) if want_dT else (out[0], out[1])


def _pointing_kw(pointing):
    """pointing=True for the mixed-state calls, or nothing: without the pointing row a call is made as it always was."""
    return dict(pointing=True) if pointing else {}


def _ray_blocks_kw(ray_blocks):
    """ray_blocks= for the mixed-state calls, or nothing: left at None a call is made as it always was."""
    return {} if ray_blocks is None else dict(ray_blocks=bool(ray_blocks))


class LevelFactored(object):
    """The level-factored route as one object: the pair tables of a LineSet on a set of (P, T) rows (LineSet.glevel_pairs;
    with dT also at T + dT, region boundaries frozen at T) and the combine for any number of LOS steps on those rows
    (glevel_combine).  The reference's own structure (make_abscoeff_isomolec: G spectra per (P, T) through
    calc_shapes_lines + add_PT, spect_main_module.py:1963-1990, then the population loop :2036-2106): line shapes are
    evaluated once per (P, T) row however many steps / SZA sets / vibrational-temperature states share it -- a 3-D path
    whose kinetic temperature lives on (latitude box, altitude) and whose vibrational temperatures follow the local
    SZA (radtran_3Dvs2D_sza30-80_test.py:66-116) has ~10x more steps than rows.

    Worth it when rows are shared: the tables cost ~3.7 folded ops per 80 rows (24 output spectra instead of 2: twelve
    passes over sub-linesets, tools/glevel_probe.py), a folded op per step costs 1 per 80 steps."""

    def __init__(self, ls, temps_rows, press_rows, dT=None, g_lo=0, g_hi=None, linear_weights=True):
        """dT: also build the tables at T + dT for the temperature derivative of `steps` -- region boundaries frozen at
        T and (linear_weights, default) the line weights linearised about T, so that (A(T + dT) - A(T)) / dT is
        sum_i w_i' y_i(T + dT) + sum_i w_i (y_i(T + dT) - y_i(T)) / dT: the weights' part exact, only the shapes
        differenced -- their dependence on T is weak (d ln y / d T ~ 1 / 2T; ~ n / T where the Lorentz width decides) and
        smooth, so dT = 0.05 K carries 1e-4 (Doppler layers) to 3.5e-4 (Lorentz layers, 80 hPa and more) of truncation
        (tests/test_frozen_reference_host.py, against a smooth derivative of the CPU reference) where the exact-weight
        quotient needed 0.002 K and sat on the reference's single-precision staircase (1e-7 |c| / dT = 1e-3 of the
        derivative)."""
        self.ls = ls
        self.dT = dT
        self._shard, self._linear = (g_lo, g_hi), linear_weights
        self.tab = self.tab_dT = None
        self.rebuild(temps_rows, press_rows)

    def rebuild(self, temps_rows, press_rows):
        """New (P, T) rows (a retrieval iteration that moved the temperatures): the tables are rebuilt IN PLACE when the
        number of rows is the same -- 6 GB per build at configs[3] size stay out of the allocator."""
        ls, (g_lo, g_hi) = self.ls, self._shard
        self.temps = np.ascontiguousarray(temps_rows, dtype=np.float64)
        self.press = np.ascontiguousarray(press_rows, dtype=np.float64)
        keep = self.tab is not None and self.tab.shape[2] == self.temps.size
        self.tab = ls.glevel_pairs(self.temps, self.press, g_lo=g_lo, g_hi=g_hi, out=self.tab if keep else None)
        if self.dT:
            ls.set_bounds_temps(self.temps, linear_weights=self._linear)
            try:
                self.tab_dT = ls.glevel_pairs(self.temps + self.dT, self.press, g_lo=g_lo, g_hi=g_hi,
                                              out=self.tab_dT if keep and self.tab_dT is not None else None)
            finally:
                ls.set_bounds_temps(None)
        return self

    @staticmethod
    def unique_rows(temps, press):
        """(T_rows, P_rows, step_row): the distinct (P, T) couples of a list of steps and every step's row."""
        pt = np.stack([np.asarray(press, float), np.asarray(temps, float)], axis=1)
        rows, inv = np.unique(pt, axis=0, return_inverse=True)
        return rows[:, 1].copy(), rows[:, 0].copy(), np.asarray(inv, np.int32).reshape(-1)

    def steps(self, step_row, tvib=None, q_part=None, derivative=False, out=None):
        """(abs, emi) [n_steps, n_pts] of the steps (each on table row step_row[s], vibrational temperatures tvib
        [n_levels, n_steps], None = LTE); derivative=True: ((abs, emi), (d abs / d T, d emi / d T)), needs dT."""
        step_row = np.ascontiguousarray(step_row, dtype=np.int32)
        T = self.temps[step_row]
        if not derivative:
            return glevel_combine(self.tab, step_row, self.ls.level_populations(T, tvib=tvib, q_part=q_part), out=out)
        if self.tab_dT is None:
            raise ValueError("LevelFactored was built without dT: no temperature derivative")
        pop, dpop = self.ls.level_populations(T, tvib=tvib, q_part=q_part, derivative=True)
        return glevel_combine(self.tab, step_row, pop, tab_dT=self.tab_dT, dpop=dpop, dT=self.dT, out=out)

    def tvib_jacobian(self, coeffs, los, step_row, tvib, par_level, par_w, gas=0, q_part=None, grid=None, want_rad=True):
        """(rad | None, jac [n_rays, n_par, n_pts]): d rad / d x_p for vibrational-temperature parameters,
        Tvib_L[r] = tvib[L, r] + sum_p par_w[p, r] x_p with L = par_level[p], on the coefficient rows r of `coeffs` --
        what steps(step_row, tvib=tvib) returned (one gas) or the stack of all gases with this one at index `gas`.
        par_w [n_par, n_steps] (level_node_weights on the rows' altitudes).  Exact and from the resident tables: the
        coefficients are linear in the populations, d pop_L / d Tvib_L = pop_L c2 E_L / Tvib_L^2
        (LineSet.level_populations_dtvib), Q(T) does not move (limb_rays_level_jacobian).  Honours the object's
        spectral shard (a Planck initial intensity is taken on grid[g_lo:])."""
        step_row = np.ascontiguousarray(step_row, dtype=np.int32)
        par_level = np.ascontiguousarray(par_level, dtype=np.int32).reshape(-1)
        par_w = np.asarray(par_w, dtype=np.float64)
        if par_w.shape != (par_level.size, step_row.size):
            raise ValueError("par_w must be [n_par, n_steps]")
        n_lev = self.ls.level_energies.size
        if par_level.size and (par_level.min() < 0 or par_level.max() >= max(n_lev, 1)):
            raise ValueError("par_level out of range")
        dpop = self.ls.level_populations_dtvib(self.temps[step_row], tvib, q_part=q_part)      # [n_steps, n_levels]
        par_c = par_w * dpop.T[par_level]
        return limb_rays_level_jacobian(coeffs, los, self.tab, step_row, par_level, par_c, gas=gas, grid=grid,
                                        g_lo=int(self._shard[0]), want_rad=want_rad)

    def state_jacobian(self, coeffs, los, step_row, tvib, par_level, par_w_level, par_gas=None, par_w_col=None, gas=0,
                       q_part=None, grid=None, want_rad=True, dcoeffs=None, par_w_temp=None, pointing=False, ray_blocks=None):
        """(rad | None, jac [n_rays, n_col + n_lev (+ n_row), n_pts]): d rad / d x for a mixed state vector in one pass
        (limb_rays_state_jacobian): first the VMR-profile parameters par_gas / par_w_col of limb_rays_jacobian (any gas
        of the batch, this one included; None: no such parameter), then the vibrational-temperature parameters
        par_level / par_w_level of tvib_jacobian, par_c = par_w_level * d pop / d Tvib formed exactly as there (an empty
        par_level: only column parameters).  dcoeffs and par_w_temp [n_row, n_steps] (both or neither): then the
        kinetic-temperature parameters, T[r] = T0[r] + sum_p par_w_temp[p, r] x_p, through the derivative spectra
        dcoeffs of every gas of the batch on the coefficient rows (this gas's: steps(..., derivative=True); the columns
        held fixed).  Honours the object's spectral shard.  pointing=True: the pointing row behind the state's
        (limb_rays_state_jacobian)."""
        step_row, par_level, par_c = self._state_level_args(step_row, tvib, par_level, par_w_level, q_part)
        return limb_rays_state_jacobian(coeffs, los, par_gas=par_gas, par_w=par_w_col, tab=self.tab, coef_row=step_row,
                                        par_level=par_level, par_c=par_c, gas=gas, grid=grid, g_lo=int(self._shard[0]),
                                        want_rad=want_rad, dcoeffs=dcoeffs, par_t=par_w_temp, **_ray_blocks_kw(ray_blocks),
                                        **_pointing_kw(pointing))

    def _state_level_args(self, step_row, tvib, par_level, par_w_level, q_part):
        """(step_row, par_level, par_c) of state_jacobian / state_bands: par_c = par_w_level * d pop / d Tvib, formed as in
        tvib_jacobian (None without level parameters)."""
        step_row = np.ascontiguousarray(step_row, dtype=np.int32)
        par_level = np.ascontiguousarray(par_level, dtype=np.int32).reshape(-1)
        par_w = np.zeros((0, step_row.size)) if par_level.size == 0 else np.asarray(par_w_level, dtype=np.float64)
        if par_w.shape != (par_level.size, step_row.size):
            raise ValueError("par_w_level must be [n_lev, n_steps]")
        n_lev = self.ls.level_energies.size
        if par_level.size and (par_level.min() < 0 or par_level.max() >= max(n_lev, 1)):
            raise ValueError("par_level out of range")
        par_c = None
        if par_level.size:
            dpop = self.ls.level_populations_dtvib(self.temps[step_row], tvib, q_part=q_part)  # [n_steps, n_levels]
            par_c = par_w * dpop.T[par_level]
        return step_row, par_level, par_c

    def state_bands(self, coeffs, los, step_row, tvib, par_level, par_w_level, grid, centers_nm, widths_nm, par_gas=None,
                    par_w_col=None, gas=0, q_part=None, dcoeffs=None, par_w_temp=None, out_units="Wm2", n_sigma=5.0, fov=None,
                    instrument=False, pointing=False, ils=None, ray_blocks=None):
        """state_jacobian on the instrument's bands in one library call (limb_rays_state_bands): numpy [n_rays | n_rays / 3,
        1 + n_par, n_bands], row 0 the radiance, row 1 + p the derivative to parameter p (VMR-profile, vibrational-
        temperature, kinetic-temperature parameters, as state_jacobian orders them); no hi-res spectrum is written.  The
        parameters' arguments and their errors are state_jacobian's; the bands' (and fov) those of limb_rays_state_bands.
        Honours the object's spectral shard: partial band integrals then (`grid` is the whole grid).  instrument=True: the
        two instrument rows behind the parameters' (limb_rays_state_bands); pointing=True: the pointing row in front of them.
        ils: an ILS, the bands' tabulated line shape."""
        step_row, par_level, par_c = self._state_level_args(step_row, tvib, par_level, par_w_level, q_part)
        return limb_rays_state_bands(coeffs, los, grid, centers_nm, widths_nm, par_gas=par_gas, par_w=par_w_col, tab=self.tab,
                                     coef_row=step_row, par_level=par_level, par_c=par_c, gas=gas, dcoeffs=dcoeffs,
                                     par_t=par_w_temp, out_units=out_units, n_sigma=n_sigma, fov=fov,
                                     g_lo=int(self._shard[0]), instrument=instrument, ils=ils, **_ray_blocks_kw(ray_blocks),
                                     **_pointing_kw(pointing))

    def level_radiances(self, coeffs, los, step_row, tvib, levels=None, weights=None, gas=0, q_part=None, grid=None,
                        gas_parts=True):
        """(rad, parts [n_rays, n_part + 1, n_pts], labels): the radiance budget of the batch by the levels of this gas
        (limb_rays_parts) on the coefficient rows of `coeffs` -- what steps(step_row, tvib=tvib) returned (one gas) or the
        stack of all gases with this one at index `gas`.  Part i is the radiance level levels[i] emits (None: every
        level), its share of the emission being pop_L[r] E_L[row[r]] with the populations of level_populations (tvib
        None: LTE); weights [n_steps] or [n_levels_asked, n_steps] multiplies them, e.g. the mask of an altitude band on
        the rows' altitudes (a level may be asked for several times, once per band).  gas_parts: then a part per gas of
        the batch (its whole emission).  The last row is the background (the initial intensity, attenuated).  labels:
        ('level', L) per level part, ('gas', g) per gas part, ('background',).  Honours the object's spectral shard."""
        step_row = np.ascontiguousarray(step_row, dtype=np.int32)
        n_lev = max(self.ls.level_energies.size, 1)
        levels = np.arange(n_lev, dtype=np.int32) if levels is None else np.ascontiguousarray(levels, dtype=np.int32).reshape(-1)
        if levels.size and (levels.min() < 0 or levels.max() >= n_lev):
            raise ValueError("level out of range")
        pop = self.ls.level_populations(self.temps[step_row], tvib=tvib, q_part=q_part)       # [n_steps, n_levels]
        part_c = pop.T[levels]
        if weights is not None:
            w = np.asarray(weights, dtype=np.float64)
            if w.shape not in ((step_row.size,), (levels.size, step_row.size)):
                raise ValueError("weights must be [n_steps] or [n_levels_asked, n_steps]")
            part_c = part_c * w
        n_gp = los.n_gas if gas_parts else 0
        part_gas = np.concatenate([np.full(levels.size, gas), np.arange(n_gp)]).astype(np.int32)
        part_level = np.concatenate([levels, np.full(n_gp, -1)]).astype(np.int32)
        part_c = np.concatenate([part_c, np.zeros((n_gp, step_row.size))])
        rad, parts = limb_rays_parts(coeffs, los, part_gas, part_level, part_c=part_c, tab=self.tab, coef_row=step_row,
                                     gas=gas, grid=grid, g_lo=int(self._shard[0]))
        labels = [("level", int(L)) for L in levels] + [("gas", g) for g in range(n_gp)] + [("background",)]
        return rad, parts, labels


class LevelFactoredSet(object):
    """Several LevelFactored of one batch -- two non-LTE emitters in one window -- for the mixed-state calls that take the
    vibrational-temperature parameters of all of them in ONE pass over each ray (limb_rays_state_jacobian /
    limb_rays_state_bands with level_gases).  members: [(lf, gas, step_row, tvib), ...] or with a fifth item q_part: a
    LevelFactored, its gas's index in the batch, the table row of every coefficient row and the vibrational temperatures
    [n_levels, n_steps] its coefficients in `coeffs` were combined with.  Level parameter p belongs to member par_lgas[p]
    and to its level par_level[p]; par_c is formed per member exactly as LevelFactored.state_jacobian forms it
    (_state_level_args: the populations' Tvib derivative times the node weights).  All members share the spectral shard.
    At most MAX_MEMBERS (four) members, whose gases may be any of the batch's up to eight (max_gases())."""

    MAX_MEMBERS = 4   # the level gases of one state call (kLevelGasMax)

    def __init__(self, members):
        self.members = [tuple(m) + (None,) * (5 - len(m)) for m in members]
        if not self.members:
            raise ValueError("LevelFactoredSet needs at least one (lf, gas, step_row, tvib)")
        if len(self.members) > self.MAX_MEMBERS:
            raise ValueError("LevelFactoredSet: %d members, at most %d gases of a batch are level-factored"
                             % (len(self.members), self.MAX_MEMBERS))
        if len({m[0]._shard for m in self.members}) != 1:
            raise ValueError("the LevelFactored of a set must share their spectral shard")
        if len({int(m[1]) for m in self.members}) != len(self.members):
            raise ValueError("a gas is named twice")

    def _args(self, par_lgas, par_level, par_w_level):
        par_lgas = np.ascontiguousarray(par_lgas, dtype=np.int32).reshape(-1)
        par_level = np.ascontiguousarray(par_level, dtype=np.int32).reshape(-1)
        if par_lgas.size != par_level.size:
            raise ValueError("par_lgas must be [n_lev], one member per level parameter")
        if par_lgas.size and (par_lgas.min() < 0 or par_lgas.max() >= len(self.members)):
            raise ValueError("par_lgas out of range")
        n_steps = np.asarray(self.members[0][2]).size
        par_w = np.zeros((0, n_steps)) if par_level.size == 0 else np.asarray(par_w_level, dtype=np.float64)
        if par_w.shape != (par_level.size, n_steps):
            raise ValueError("par_w_level must be [n_lev, n_steps]")
        par_c, gases = np.zeros((par_level.size, n_steps)), []
        for k, (lf, gas, step_row, tvib, q_part) in enumerate(self.members):
            idx = np.nonzero(par_lgas == k)[0]
            if np.asarray(step_row).size != n_steps:
                raise ValueError("the members' step_row must have one length, the coefficient rows of the batch")
            step_row, _, pc = lf._state_level_args(step_row, tvib, par_level[idx], par_w[idx], q_part)
            if idx.size:
                par_c[idx] = pc
            gases.append((int(gas), lf.tab, step_row))
        return gases, par_lgas, par_level, par_c

    def state_jacobian(self, coeffs, los, par_lgas, par_level, par_w_level, par_gas=None, par_w_col=None, grid=None,
                       want_rad=True, dcoeffs=None, par_w_temp=None, pointing=False, ray_blocks=None):
        """LevelFactored.state_jacobian for the members' vibrational-temperature parameters together: (rad | None, jac
        [n_rays, n_col + n_lev (+ n_row), n_pts]), the rows in the caller's order; pointing=True: the pointing row behind."""
        gases, par_lgas, par_level, par_c = self._args(par_lgas, par_level, par_w_level)
        return limb_rays_state_jacobian(coeffs, los, par_gas=par_gas, par_w=par_w_col, par_level=par_level, par_c=par_c,
                                        grid=grid, g_lo=int(self.members[0][0]._shard[0]), want_rad=want_rad, dcoeffs=dcoeffs,
                                        par_t=par_w_temp, level_gases=gases, par_lgas=par_lgas, **_ray_blocks_kw(ray_blocks),
                                        **_pointing_kw(pointing))

    def state_bands(self, coeffs, los, par_lgas, par_level, par_w_level, grid, centers_nm, widths_nm, par_gas=None,
                    par_w_col=None, dcoeffs=None, par_w_temp=None, out_units="Wm2", n_sigma=5.0, fov=None, instrument=False,
                    pointing=False, ils=None, ray_blocks=None):
        """LevelFactored.state_bands for the members' vibrational-temperature parameters together: numpy [n_rays | n_rays / 3,
        1 + n_par, n_bands]; instrument=True: [.., 1 + n_par + 2, n_bands], the two instrument rows last; pointing=True:
        the pointing row behind the parameters'; ils: an ILS, the bands' tabulated line shape."""
        gases, par_lgas, par_level, par_c = self._args(par_lgas, par_level, par_w_level)
        return limb_rays_state_bands(coeffs, los, grid, centers_nm, widths_nm, par_gas=par_gas, par_w=par_w_col,
                                     par_level=par_level, par_c=par_c, dcoeffs=dcoeffs, par_t=par_w_temp, out_units=out_units,
                                     n_sigma=n_sigma, fov=fov, g_lo=int(self.members[0][0]._shard[0]), level_gases=gases,
                                     par_lgas=par_lgas, instrument=instrument, ils=ils, **_ray_blocks_kw(ray_blocks),
                                     **_pointing_kw(pointing))


def level_node_weights(nodes, alt):
    """par_w [n_nodes, n_rows] of one level's vibrational-temperature profile on the coefficient rows: the triangular
    masks of LinearProfile_1D_new (spect_main_module.alt_triangle: 1 at the node, linear to 0 at its neighbours, the
    first / last node continued with 1 below / above) at the rows' altitudes `alt` -- a profile that is linear between
    the nodes `nodes` (increasing, at least two).  Inside the node range the weights of a row sum to one."""
    from . import spect_main_module as smm
    nodes = [float(v) for v in nodes]
    if len(nodes) < 2 or any(b <= a for a, b in zip(nodes[:-1], nodes[1:])):
        raise ValueError("at least two increasing node altitudes")
    prof = smm.LinearProfile_1D_new("tvib", np.asarray(alt, dtype=float).reshape(-1), nodes, np.zeros(len(nodes)),
                                    np.ones(len(nodes)))
    return np.ascontiguousarray(prof.mask_matrix())


def set_timing(on):
    """0: no timing events in the coefficient op (host-bound loops: small shards); last_kernel_ms is then unavailable.
    2: also around the recursion of the retrieval's forward model (LimbLOS.last_forward_kernel_ms)."""
    check(lib.sr_set_timing(int(on)), "sr_set_timing")


def set_counting(on):
    """1: the next coefficient ops run the counting instantiations (executed-work accounting, untimed)."""
    check(lib.sr_set_counting(int(bool(on))), "sr_set_counting")


def radiance_rays(abs_c, emi_c, seg_off, seg_layer, seg_col, rad0=None):
    """Limb radiance recursion for a batch of rays (include/spectrobot_hip.h).
    abs_c/emi_c: CUDA float64 [n_layers, n_pts]; returns CUDA float64 [n_rays, n_pts]."""
    assert abs_c.is_cuda and abs_c.dtype == torch.float64 and abs_c.is_contiguous()
    assert emi_c.shape == abs_c.shape and emi_c.is_contiguous()
    n_layers, n_pts = abs_c.shape
    seg_off, op = _i(seg_off)
    seg_layer, lp = _i(seg_layer)
    seg_col, cp = _d(seg_col)
    n_rays = seg_off.size - 1
    if rad0 is None:
        rad = torch.empty((n_rays, n_pts), dtype=torch.float64, device="cuda")
        init = 0
    else:
        rad = rad0
        assert rad.shape == (n_rays, n_pts) and rad.is_contiguous()
        init = 1
    check(lib.sr_radiance_rays_dev(C.c_void_p(abs_c.data_ptr()), C.c_void_p(emi_c.data_ptr()), n_layers, n_pts,
                                   n_rays, op, lp, cp, init, C.c_void_p(rad.data_ptr()), _stream_ptr()),
          "sr_radiance_rays_dev")
    return rad


class _ParHandle(object):
    def __init__(self, h, keep=None):
        self.h, self.keep = h, keep     # keep: the arrays an identity key refers to (their ids stay theirs while kept)


def _array_key(a):
    """Key of an array for the resident-handle cache: a READ-ONLY ndarray that OWNS its data cannot change under its
    identity (and the cache entry keeps it alive, so the id is not re-used): ("id", id(a)), free; anything else by content
    (_content_key) -- a read-only view too: its base may be writable, and an edit through the base changes what the view
    shows.  retrieval.LimbScene.profile_weights hands out read-only arrays that own their data: a retrieval iteration then
    pays no hashing of its 60 000-entry weight table (60-100 us of a 480 us iteration)."""
    if isinstance(a, np.ndarray) and a.base is None and a.flags.owndata and not a.flags.writeable:
        return ("id", id(a))
    return _content_key(a)


_KEY_MULT = np.uint64(0x9E3779B97F4A7C15)   # an odd constant (2^64 / the golden ratio): spreads 2 pos + 1 over the word


def _content_key(a):
    """A key for an array's CONTENT (dtype, shape, bytes hashed): identity says nothing about an array edited in place or
    about a new array that got a dead one's id."""
    a = np.ascontiguousarray(a)
    if a.nbytes <= 4096 or a.nbytes % 8:
        return (a.dtype.str, a.shape, a.tobytes())
    # large tables (a retrieval's parameter weights, every iteration): two vectorised reductions over the 64-bit words
    # -- xor and a position-weighted wrapped sum -- instead of a cryptographic hash (0.5 ms per call).  Every position
    # has its own odd multiplier, (2 pos + 1) K mod 2^64: two words that change places move the sum by
    # (f(a) - f(b)) 2 (i - j) K, which is 0 only if f(a) - f(b) is a multiple of 2^63 / (i - j)'s power of two.  f folds
    # a word's upper half into its lower (a bijection), so that x and -x -- words that differ in bit 63 alone -- do not
    # meet that condition as neighbours.
    w = a.reshape(-1).view(np.uint64)
    mult = (np.arange(w.size, dtype=np.uint64) * np.uint64(2) + np.uint64(1)) * _KEY_MULT
    f = w ^ (w >> np.uint64(31))
    return (a.dtype.str, a.shape, int(np.bitwise_xor.reduce(w)), int((f * mult).sum(dtype=np.uint64)))


class LimbLOS(object):
    """A batch of lines of sight for the device LOS pipeline (sr_los_desc): per ray the segments it crosses,
    per segment the layer whose coefficients apply and the LOS sample points (path coordinate x [cm], number
    density nd [cm^-3], VMR of every gas) over which the Curtis-Godson column is integrated on the device.

    seg_off [n_rays+1], seg_layer [n_seg], pt_off [n_seg+1], x / nd [n_pt], vmr [n_gas, n_pt].
    Options as at the reference's call sites: LOS_order ('photon' | 'observer'), solo_absorption,
    initial_intensity: None, a temperature (Planck source, Calc_BB) or 'rad0' (given per call).
    path (optional, limb rays of geometry.limb_los(path=True) only): dict(alt=, dx=, dalt=), [n_pt] each -- the sample
    points' altitudes [km] and the derivatives of x [cm / km] and of the altitude to the ray's own tangent altitude; kept
    with the geometry, it is what the calls with pointing=True and los_columns_dz need."""

    def __init__(self, seg_off, seg_layer, pt_off, x, nd, vmr, col_scale=None, LOS_order='photon',
                 solo_absorption=False, initial_temperature=None, path=None):
        # (copies: the object is the geometry as given -- its device-resident form is built once, see handle())
        self.seg_off, self._so = _i(np.array(seg_off))
        self.seg_layer, self._sl = _i(np.array(seg_layer))
        self.pt_off, self._po = _i(np.array(pt_off))
        self.x, self._x = _d(np.array(x))
        self.nd, self._nd = _d(np.array(nd))
        self.vmr, self._v = _d(np.atleast_2d(np.array(vmr)))
        self.n_rays, self.n_gas = self.seg_off.size - 1, self.vmr.shape[0]
        self.n_seg, self.n_pt = self.seg_layer.size, self.x.size
        if self.vmr.shape[1] != self.n_pt or self.nd.size != self.n_pt or self.pt_off.size != self.n_seg + 1:
            raise ValueError("inconsistent LOS arrays")
        self.col_scale, self._cs = (None, None) if col_scale is None else _d(col_scale)
        if LOS_order not in ('photon', 'observer'):
            raise ValueError("LOS_order must be 'photon' or 'observer'")
        self.LOS_order, self.solo_absorption, self.initial_temperature = LOS_order, bool(solo_absorption), initial_temperature
        self._handles = {}      # insertion-ordered: least recently used first (see _keep)
        self.path = None
        if path is not None:
            self.path = tuple(_d(np.array(path[k])) for k in ("alt", "dx", "dalt"))
            if any(a.shape != (self.n_pt,) for a, _ in self.path):
                raise ValueError("path arrays must be [n_pt]")

    MAX_HANDLES = 8   # resident forms kept per batch: each holds pinned and device memory until it is destroyed

    def _keep(self, key, ent):
        """Insert / refresh an entry of the bounded handle cache; the least recently used forms are destroyed."""
        self._handles.pop(key, None)
        self._handles[key] = ent
        while len(self._handles) > self.MAX_HANDLES:
            old = self._handles.pop(next(iter(self._handles)))
            lib.sr_los_destroy(getattr(old, "h", old))
        return ent

    def handle(self, n_layers, grid=None, rad0=False):
        """The batch resident on the device (sr_los_create): staged, its columns integrated and the folded sweep's
        records packed once per (n_layers, grid, rad0); limb_rays and LineSet.limb_step then only launch.  The
        object IS the geometry it was built from: its arrays were copied at construction.  New VMRs go through
        set_vmr() (which updates the resident forms); other paths need a new LimbLOS."""
        gp = None if (grid is None or self.initial_temperature is None or rad0) else grid_params(grid)[:2]
        key = (int(n_layers), gp, bool(rad0))
        h = self._handles.get(key)
        if h is None:
            d = self.desc(grid, 0, rad0=rad0)
            h = C.c_void_p()
            check(lib.sr_los_create(C.byref(d), int(n_layers), C.byref(h)), "sr_los_create")
        return self._keep(key, h)

    def handle_par(self, n_layers, par_gas, par_w, grid=None, rad0=False):
        """handle() with the column parameters (par_gas [n_par], par_w [n_par, n_pt]) staged alongside
        (sr_los_create_par): the batch of a retrieval.  Keyed on the two arrays' CONTENT (a hash of their bytes: a
        caller that builds par_w afresh every iteration finds its batch again, an in-place edit makes a new one) -- or,
        for read-only arrays, on their identity (_array_key); at most MAX_HANDLES resident forms are kept, the least
        recently used is destroyed."""
        gp = None if (grid is None or self.initial_temperature is None or rad0) else grid_params(grid)[:2]
        pg_a, pg = _i(par_gas)
        pw_a, pw = _d(par_w)
        if pw_a.shape != (pg_a.size, self.n_pt):
            raise ValueError("par_w must be [n_par, n_pt]")
        key = (int(n_layers), gp, bool(rad0), _array_key(par_gas), _array_key(par_w))
        ent = self._handles.get(key)
        if ent is None:
            d = self.desc(grid, 0, rad0=rad0)
            h = C.c_void_p()
            check(lib.sr_los_create_par(C.byref(d), int(n_layers), pg_a.size, pg, pw, C.byref(h)), "sr_los_create_par")
            ent = _ParHandle(h, keep=(par_gas, par_w))
        return self._keep(key, ent).h

    def last_forward_kernel_ms(self, n_layers, par_gas, par_w, grid=None):
        """HIP-event time [ms] of the recursion (record packing + the one-sweep kernel with the bands in its epilogue) of
        the most recent retrieval_forward / _step / _loop on this batch with these parameters, made under set_timing(2)
        (sr_los_last_kernel_ms)."""
        ms = C.c_float(0.0)
        check(lib.sr_los_last_kernel_ms(self.handle_par(n_layers, par_gas, par_w, grid), C.byref(ms)), "sr_los_last_kernel_ms")
        return float(ms.value)

    def refresh_columns(self):
        """Integrate the Curtis-Godson columns of every resident form of the batch again, on the device, from the staged
        sample points (sr_los_refresh_columns: launches only)."""
        for h in self._handles.values():
            check(lib.sr_los_refresh_columns(getattr(h, "h", h), _stream_ptr()), "sr_los_refresh_columns")

    def set_vmr(self, vmr):
        """New VMRs [n_gas, n_pt] at the sample points (the next iteration of a retrieval): the host copy and every
        resident form of the batch (sr_los_set_vmr: one small copy + the column kernel; nothing else is re-staged)."""
        v = np.ascontiguousarray(np.atleast_2d(vmr), dtype=np.float64)
        if v.shape != self.vmr.shape:
            raise ValueError("vmr must be [n_gas, n_pt]")
        if self.LOS_order != 'photon' and self._handles:
            # sr_los_set_vmr refuses observer-order batches (their sample points are re-listed): checked BEFORE the
            # host copy changes, so that it and the resident forms never disagree -- drop the forms, they are rebuilt
            self.close()
        self.vmr[...] = v
        for h in self._handles.values():
            check(lib.sr_los_set_vmr(getattr(h, "h", h), self._v, _stream_ptr()), "sr_los_set_vmr")

    def close(self):
        for h in getattr(self, "_handles", {}).values():
            if lib is not None:
                lib.sr_los_destroy(getattr(h, "h", h))
        self._handles = {}

    __del__ = close

    def desc(self, grid=None, g_lo=0, rad0=False):
        d = _lib.LosDesc()
        d.n_rays, d.n_gas = self.n_rays, self.n_gas
        d.seg_off, d.seg_layer, d.pt_off, d.x, d.nd, d.vmr = self._so, self._sl, self._po, self._x, self._nd, self._v
        d.col_scale = self._cs
        d.los_order = 0 if self.LOS_order == 'photon' else 1
        d.solo_absorption = int(self.solo_absorption)
        d.init_mode, d.t_init, d.w0, d.step, d.g_lo = 0, 0.0, 0.0, 0.0, int(g_lo)
        if rad0:
            d.init_mode = 1
        elif self.initial_temperature is not None:
            if grid is None:
                raise ValueError("a Planck initial intensity needs the spectral grid")
            w0, step, _ = grid_params(grid)
            d.init_mode, d.t_init, d.w0, d.step = 2, float(self.initial_temperature), w0, step
        return d

    def path_desc(self):
        """The sr_los_path of the batch; ValueError for a batch built without `path`."""
        if self.path is None:
            raise ValueError("the pointing derivative needs a LimbLOS built with path= (geometry.limb_los(path=True))")
        p = _lib.LosPath()
        p.alt, p.dx_dz, p.dalt_dz = (ptr for _, ptr in self.path)
        return p

    def columns(self):
        """[n_gas, n_seg] Curtis-Godson columns (curgod_fort_2 per segment, on the device)."""
        out = np.zeros((self.n_gas, self.n_seg))
        d = self.desc()
        check(lib.sr_los_columns(C.byref(d), out.ctypes.data_as(dp)), "sr_los_columns")
        return out


def los_columns_dz(los):
    """[n_gas, n_seg] d column / d z_t of a limb batch built with path= (sr_los_columns_dz): the derivative of
    LimbLOS.columns() to every ray's own tangent altitude [per km], the crossed shells held fixed, on the device.
    Photon order only; a batch without path raises ValueError."""
    p = los.path_desc()
    out = np.zeros((los.n_gas, los.n_seg))
    d = los.desc()
    check(lib.sr_los_columns_dz(C.byref(d), C.byref(p), out.ctypes.data_as(dp)), "sr_los_columns_dz")
    return out


def gas_stack(coeffs):
    """The gases' coefficient tables stacked once, [n_gas, n_layers, n_pts] x 2, for callers that pass the same tables to
    many limb_rays* calls (a retrieval loop whose coefficients do not change: the stacking copies every table)."""
    return _gas_stack(coeffs)


def _gas_stack(coeffs):
    """[(abs, emi)] per gas, one (abs, emi) pair or an already stacked pair (gas_stack) -> contiguous CUDA
    [n_gas, n_layers, n_pts] x 2."""
    if isinstance(coeffs[0], torch.Tensor):
        if coeffs[0].dim() == 3:
            a, e = coeffs
            assert a.is_cuda and a.dtype == torch.float64 and e.shape == a.shape and a.is_contiguous() and e.is_contiguous()
            return a, e
        coeffs = [coeffs]
    a = torch.stack([c[0] for c in coeffs]).contiguous() if len(coeffs) > 1 else coeffs[0][0].contiguous()[None]
    e = torch.stack([c[1] for c in coeffs]).contiguous() if len(coeffs) > 1 else coeffs[0][1].contiguous()[None]
    assert a.is_cuda and a.dtype == torch.float64 and e.shape == a.shape
    return a, e


def max_gases(folded=False):
    """The gases a LimbLOS batch may carry (sr_limb_max_gases): 8 for limb_rays and every state call
    (limb_rays_state_jacobian, limb_rays_state_bands, limb_rays_level_jacobian, LevelFactored / LevelFactoredSet); with
    folded=True, 4: limb_rays_jacobian, limb_rays_jacobians, limb_rays_layer_jacobian, limb_rays_parts,
    retrieval_forward, retrieval_step and retrieval_loop, whose kernels keep four gas slots in their packed records."""
    return int(lib.sr_limb_max_gases(1 if folded else 0))


def _four_gas_call(call, los):
    """The calls of the folded-limit kernels refuse a larger batch here, before any device call."""
    limit = max_gases(folded=True)
    if los.n_gas > limit:
        raise ValueError("%s: a batch of %d gases, the call takes at most max_gases(folded=True) = %d (limb_rays and the "
                         "state calls take %d)" % (call, los.n_gas, limit, max_gases()))


def limb_rays(coeffs, los, grid=None, g_lo=0, rad0=None, resident=True):
    """Radiances [n_rays, n_pts] of a LimbLOS batch through the gases' coefficients: columns per segment on the device,
    then the recursion.  coeffs: (abs, emi) or [(abs, emi)] per gas, CUDA [n_layers, n_pts] each.  rad0: CUDA
    [n_rays, n_pts] initial intensity (overwritten).  resident (default): through the batch's device-resident form
    (LimbLOS.handle -> sr_limb_rays_los_dev); False: staged per call (sr_limb_rays_dev)."""
    a, e = _gas_stack(coeffs)
    n_gas, n_layers, n_pts = a.shape
    if n_gas != los.n_gas:
        raise ValueError("%d coefficient sets for %d gases" % (n_gas, los.n_gas))
    rad = rad0 if rad0 is not None else torch.empty((los.n_rays, n_pts), dtype=torch.float64, device="cuda")
    assert rad.shape == (los.n_rays, n_pts) and rad.is_contiguous()
    if resident:   # the LOS staged, its columns and plan made once (sr_los_create); this call only launches
        h = los.handle(n_layers, grid, rad0=rad0 is not None)
        check(lib.sr_limb_rays_los_dev(a.data_ptr(), e.data_ptr(), n_layers, n_pts, h, int(g_lo), rad.data_ptr(), _stream_ptr()),
              "sr_limb_rays_los_dev")
        return rad
    d = los.desc(grid, g_lo, rad0=rad0 is not None)
    check(lib.sr_limb_rays_dev(C.c_void_p(a.data_ptr()), C.c_void_p(e.data_ptr()), n_layers, n_pts, C.byref(d),
                               C.c_void_p(rad.data_ptr()), _stream_ptr()), "sr_limb_rays_dev")
    return rad


def limb_rays_jacobian(coeffs, los, par_gas, par_w, grid=None, g_lo=0, rad0=None, joint=False, resident=False):
    """Radiances and d rad / d x_p [n_rays, n_par, n_pts] for VMR-profile parameters: the VMR of gas
    par_gas[p] at LOS sample point i is sum_p par_w[p, i] x_p (sr_limb_rays_jac_dev).
    joint=True: both live in ONE buffer [n_rays (1 + n_par), n_pts] -- the radiances' rows first -- which is returned
    as a third value (one hires_to_lowres call, one copy to the host, for a retrieval iteration).
    resident=True: through the batch's device-resident form with these parameter arrays (LimbLOS.handle_par, keyed on
    the arrays' identity) -- a retrieval loop that keeps its LimbLOS and calls los.set_vmr between iterations."""
    _four_gas_call("limb_rays_jacobian", los)
    a, e = _gas_stack(coeffs)
    n_gas, n_layers, n_pts = a.shape
    par_gas_in, par_w_in = par_gas, par_w
    par_gas, pg = _i(par_gas)
    par_w, pw = _d(par_w)
    n_par = par_gas.size
    if par_w.shape != (n_par, los.n_pt):
        raise ValueError("par_w must be [n_par, n_pt]")
    buf = None
    if joint:
        if rad0 is not None:
            raise ValueError("joint=True allocates the radiances itself (no rad0)")
        buf = torch.empty((los.n_rays * (1 + n_par), n_pts), dtype=torch.float64, device="cuda")
        rad, jac = buf[:los.n_rays], buf[los.n_rays:].view(los.n_rays, n_par, n_pts)
    else:
        rad = rad0 if rad0 is not None else torch.empty((los.n_rays, n_pts), dtype=torch.float64, device="cuda")
        jac = torch.empty((los.n_rays, n_par, n_pts), dtype=torch.float64, device="cuda")
    if resident:   # the batch with its parameters staged once (sr_los_create_par); VMR updates through los.set_vmr
        h = los.handle_par(n_layers, par_gas_in, par_w_in, grid, rad0=rad0 is not None)
        check(lib.sr_limb_rays_jac_los_dev(a.data_ptr(), e.data_ptr(), n_layers, n_pts, h, int(g_lo), rad.data_ptr(), jac.data_ptr(),
                                           _stream_ptr()), "sr_limb_rays_jac_los_dev")
        return (rad, jac, buf) if joint else (rad, jac)
    d = los.desc(grid, g_lo, rad0=rad0 is not None)
    check(lib.sr_limb_rays_jac_dev(C.c_void_p(a.data_ptr()), C.c_void_p(e.data_ptr()), n_layers, n_pts, C.byref(d),
                                   n_par, pg, pw, C.c_void_p(rad.data_ptr()), C.c_void_p(jac.data_ptr()),
                                   _stream_ptr()), "sr_limb_rays_jac_dev")
    return (rad, jac, buf) if joint else (rad, jac)


def fov_factors(pixel_rot):
    """[n_pix, 7] = delta, delta^3, 2 dmax^2, edge, m2, esse, has_edge of the rotated square pixels (degrees): the geometry
    factors of spect_main_module.fov_closed_form (FOV_integr_1D, spect_main_module.py:3342-3374), in its operations."""
    out = np.zeros((len(pixel_rot), 7))
    for i, rot_deg in enumerate(pixel_rot):
        rot = abs(np.deg2rad(rot_deg))
        dmax = np.sqrt(2.0) / 2.0 * np.cos(np.pi / 4 - rot)
        delta = dmax - np.sin(rot)
        esse = 1.0 / np.cos(rot)
        edge = dmax - delta
        m2 = dmax * (dmax ** 3 - delta ** 3) / 3.0 - (dmax ** 4 - delta ** 4) / 4.0
        out[i] = (delta, delta ** 3, 2.0 * dmax ** 2, edge, m2, esse, 1.0 if edge > 1e-14 * dmax else 0.0)
    return out


def retrieval_forward(coeffs, los, par_gas, par_w, x, grid, centers_nm, widths_nm, out_units="Wm2", n_sigma=5.0, g_lo=0,
                      fov=None, buf=None, ils=None):
    """The forward model of one retrieval iteration in ONE library call (sr_retrieval_forward_dev) on the batch's
    device-resident form with these parameter arrays (LimbLOS.handle_par): parameter vector x -> VMRs of the retrieved
    gases at the sample points -> columns -> radiances and parameter Jacobians -> instrument bands -> (fov: fov_factors
    of the pixels, three rays each) the closed-form field-of-view integral.  Returns numpy [n_pix or n_rays, 1 + n_par,
    n_bands]: row 0 the radiance, row 1 + p its derivative to x_p; a spectral shard (g_lo, the coefficient tables'
    width) gives its partial band integrals.  The batch's host copy of the VMRs (los.vmr) is NOT updated: call
    los.set_vmr when the loop ends.  buf: scratch from an earlier call (returned as second value).  ils: an ILS, the
    bands' tabulated line shape (as hires_to_lowres)."""
    _four_gas_call("retrieval_forward", los)
    a, e = _gas_stack(coeffs)
    n_gas, n_layers, n_pts = a.shape
    w0, step, n = grid_params(grid)
    x_a, xp = _d(x)
    n_par = x_a.size
    centers_nm, cp = _d(centers_nm)
    widths_nm, wp = _d(widths_nm)
    if widths_nm.size != centers_nm.size:
        raise ValueError("{} spectral widths for {} grid points".format(widths_nm.size, centers_nm.size))
    if not (0 <= g_lo and g_lo + n_pts <= n):
        raise ValueError("the coefficient tables cover grid points outside the grid")
    h = los.handle_par(n_layers, par_gas, par_w, grid)
    if np.asarray(par_gas).size != n_par:
        raise ValueError("x must hold one value per parameter")
    n_out = los.n_rays
    fp = None
    if fov is not None:
        fov, fp = _d(fov)
        if los.n_rays % 3 or fov.shape != (los.n_rays // 3, 7):
            raise ValueError("fov must be [n_rays / 3, 7] (three rays per pixel)")
        n_out = los.n_rays // 3
    if buf is None or buf.shape != (los.n_rays * (1 + n_par), n_pts):
        buf = torch.empty((los.n_rays * (1 + n_par), n_pts), dtype=torch.float64, device="cuda")
    out = np.empty((n_out, 1 + n_par, centers_nm.size))
    with _IlsBound(ils):
        check(lib.sr_retrieval_forward_dev(a.data_ptr(), e.data_ptr(), n_layers, n_pts, h, int(g_lo), xp, w0, step, cp, wp,
                                           centers_nm.size, float(n_sigma), _UNITS[out_units], fp, buf.data_ptr(),
                                           out.ctypes.data_as(dp), _stream_ptr()), "sr_retrieval_forward_dev")
    return out, buf


class OeProblem(object):
    """What sr_retrieval_step_dev needs of a retrieval besides the forward model, marshalled once per loop: observations,
    noise and mask of the pixels (pixel-major, band-minor, as genvec concatenates them), the inverse a-priori
    covariance, the a-priori vector, the Levenberg-Marquardt factor."""

    def __init__(self, obs, noise, mask, sa_inv, x_apriori, lambda_lm):
        self.obs, self._o = _d(np.asarray(obs, float).reshape(-1))
        self.noise, self._n = _d(np.asarray(noise, float).reshape(-1))
        self.mask = None if mask is None else np.ascontiguousarray(np.asarray(mask).reshape(-1), dtype=np.uint8)
        self.sa_inv, self._s = _d(sa_inv)
        self.x_ap, self._x = _d(x_apriori)
        n_par = self.x_ap.size
        if self.sa_inv.shape != (n_par, n_par) or self.noise.size != self.obs.size or (self.mask is not None and self.mask.size != self.obs.size):
            raise ValueError("inconsistent optimal-estimation problem")
        self.desc = _lib.OeDesc(self.obs.size, self._o, self._n,
                                None if self.mask is None else self.mask.ctypes.data_as(C.POINTER(C.c_uint8)), self._s, self._x,
                                float(lambda_lm))
        self.n_par = n_par


def retrieval_step(coeffs, los, par_gas, par_w, x, grid, centers_nm, widths_nm, oe, out_units="Wm2", n_sigma=5.0, fov=None,
                   buf=None, ils=None):
    """retrieval_forward + the rest of the iteration in the same library call (sr_retrieval_step_dev): chi square of the
    pixels against the observations and the Levenberg-Marquardt step of the optimal-estimation algebra
    (spect_main_module.inversion_algebra) on the band spectra and Jacobians the call brings to the host.  oe: OeProblem.
    Returns (out [n_pix, 1 + n_par, n_bands], chi_sum, n_used, dx [n_par], S_x, AVK [n_par, n_par], buf).  Single process
    only (a shard's band integrals are partial).  ils: as retrieval_forward."""
    _four_gas_call("retrieval_step", los)
    a, e = _gas_stack(coeffs)
    n_gas, n_layers, n_pts = a.shape
    w0, step, n = grid_params(grid)
    if n_pts != n:
        raise ValueError("retrieval_step needs the whole grid (a spectral shard's band integrals are partial)")
    x_a, xp = _d(x)
    n_par = x_a.size
    centers_nm, cp = _d(centers_nm)
    widths_nm, wp = _d(widths_nm)
    h = los.handle_par(n_layers, par_gas, par_w, grid)
    if np.asarray(par_gas).size != n_par or oe.n_par != n_par or los.n_rays % 3:
        raise ValueError("x, the parameters and the problem must agree; three rays per pixel")
    n_pix = los.n_rays // 3
    fp = None
    if fov is not None:
        fov, fp = _d(fov)
        if fov.shape != (n_pix, 7):
            raise ValueError("fov must be [n_rays / 3, 7]")
    if buf is None or buf.shape != (los.n_rays * (1 + n_par), n_pts):
        buf = torch.empty((los.n_rays * (1 + n_par), n_pts), dtype=torch.float64, device="cuda")
    out = np.empty((n_pix, 1 + n_par, centers_nm.size))
    chi, n_used = C.c_double(0.0), C.c_int32(0)
    dx, s_x, avk = np.empty(n_par), np.empty((n_par, n_par)), np.empty((n_par, n_par))
    with _IlsBound(ils):
        check(lib.sr_retrieval_step_dev(a.data_ptr(), e.data_ptr(), n_layers, n_pts, h, 0, xp, w0, step, cp, wp, centers_nm.size,
                                        float(n_sigma), _UNITS[out_units], fp, buf.data_ptr(), out.ctypes.data_as(dp),
                                        C.byref(oe.desc), C.byref(chi), C.byref(n_used), dx.ctypes.data_as(dp),
                                        s_x.ctypes.data_as(dp), avk.ctypes.data_as(dp), _stream_ptr()), "sr_retrieval_step_dev")
    return out, chi.value, n_used.value, dx, s_x, avk, buf


def retrieval_loop(coeffs, los, par_gas, par_w, x0, grid, centers_nm, widths_nm, oe, positive, n_dof_par, chi_threshold=0.01,
                   max_it=10, out_units="Wm2", n_sigma=5.0, fov=None, buf=None, ils=None):
    """The whole loop of a retrieval whose coefficient spectra stay fixed, in one library call (sr_retrieval_loop_dev):
    retrieval_step per iteration, reduced chi square, the stopping rule and the update with the positivity rule of
    spect_main_module.inversion_fast_limb.  positive [n_par] bool: constrain_positive of every parameter; n_dof_par: the
    parameters in use.  Returns (out of the last iteration [n_pix, 1 + n_par, n_bands], chi history [n_it], x history
    [n_updates + 1, n_par], stop '' | 'converged' | 'raised', S_x, AVK (None when no update was applied), buf).  ils: as
    retrieval_forward."""
    _four_gas_call("retrieval_loop", los)
    a, e = _gas_stack(coeffs)
    n_gas, n_layers, n_pts = a.shape
    w0, step, n = grid_params(grid)
    if n_pts != n:
        raise ValueError("retrieval_loop needs the whole grid (a spectral shard's band integrals are partial)")
    x_a, xp = _d(x0)
    n_par = x_a.size
    centers_nm, cp = _d(centers_nm)
    widths_nm, wp = _d(widths_nm)
    h = los.handle_par(n_layers, par_gas, par_w, grid)
    if np.asarray(par_gas).size != n_par or oe.n_par != n_par or los.n_rays % 3:
        raise ValueError("x, the parameters and the problem must agree; three rays per pixel")
    n_pix = los.n_rays // 3
    fp = None
    if fov is not None:
        fov, fp = _d(fov)
        if fov.shape != (n_pix, 7):
            raise ValueError("fov must be [n_rays / 3, 7]")
    if buf is None or buf.shape != (los.n_rays * (1 + n_par), n_pts):
        buf = torch.empty((los.n_rays * (1 + n_par), n_pts), dtype=torch.float64, device="cuda")
    pos = np.ascontiguousarray(np.asarray(positive, dtype=bool).reshape(-1), dtype=np.uint8)
    if pos.size != n_par:
        raise ValueError("positive must be [n_par]")
    max_it = int(max_it)
    lp = _lib.LoopDesc(max_it, float(chi_threshold), pos.ctypes.data_as(C.POINTER(C.c_uint8)), int(n_dof_par))
    out = np.zeros((n_pix, 1 + n_par, centers_nm.size))
    chi_hist, x_hist = np.zeros(max(max_it, 1)), np.zeros((max_it + 1, n_par))
    n_it, stop = C.c_int32(0), C.c_int32(0)
    s_x, avk = np.zeros((n_par, n_par)), np.zeros((n_par, n_par))
    with _IlsBound(ils):
        check(lib.sr_retrieval_loop_dev(a.data_ptr(), e.data_ptr(), n_layers, n_pts, h, 0, xp, w0, step, cp, wp, centers_nm.size,
                                        float(n_sigma), _UNITS[out_units], fp, buf.data_ptr(), out.ctypes.data_as(dp),
                                        C.byref(oe.desc), C.byref(lp), chi_hist.ctypes.data_as(dp), x_hist.ctypes.data_as(dp),
                                        C.byref(n_it), C.byref(stop), s_x.ctypes.data_as(dp), avk.ctypes.data_as(dp), _stream_ptr()),
              "sr_retrieval_loop_dev")
    n_upd = n_it.value if stop.value == 0 else n_it.value - 1
    return (out, chi_hist[:n_it.value].copy(), x_hist[:n_upd + 1].copy(), ["", "converged", "raised"][stop.value],
            s_x if n_upd > 0 else None, avk if n_upd > 0 else None, buf)


def limb_rays_layer_jacobian(coeffs, dcoeffs, los, grid=None, g_lo=0):
    """d rad / d (one scalar per layer) [n_rays, n_layers, n_pts]; dcoeffs like coeffs: d(abs, emi of layer k) /
    d(parameter of layer k) per gas (sr_limb_rays_jac_layer_dev)."""
    _four_gas_call("limb_rays_layer_jacobian", los)
    a, e = _gas_stack(coeffs)
    da, de = _gas_stack(dcoeffs)
    n_gas, n_layers, n_pts = a.shape
    assert da.shape == a.shape
    jac = torch.empty((los.n_rays, n_layers, n_pts), dtype=torch.float64, device="cuda")
    d = los.desc(grid, g_lo)
    check(lib.sr_limb_rays_jac_layer_dev(C.c_void_p(a.data_ptr()), C.c_void_p(e.data_ptr()), C.c_void_p(da.data_ptr()),
                                         C.c_void_p(de.data_ptr()), n_layers, n_pts, C.byref(d),
                                         C.c_void_p(jac.data_ptr()), _stream_ptr()), "sr_limb_rays_jac_layer_dev")
    return jac


def limb_rays_jacobians(coeffs, los, dcoeffs=None, par_gas=None, par_w=None, grid=None, g_lo=0, want_rad=True,
                        seg_jac_row=None, n_jac_rows=None):
    """Radiances, per-layer Jacobian (dcoeffs given: d(abs, emi of layer k)/d(scalar of layer k) per gas) and
    column-parameter Jacobian (par_gas / par_w given, as limb_rays_jacobian) in ONE pass over each ray
    (sr_limb_rays_jacobians_dev).  Returns (rad | None, jac_layer | None, jac_par | None).
    seg_jac_row [n_seg] (with n_jac_rows): the per-layer Jacobian row of every segment when it is not the segment's
    coefficient row (3-D paths: a coefficient row per LOS step, the Jacobian per altitude layer)."""
    _four_gas_call("limb_rays_jacobians", los)
    a, e = _gas_stack(coeffs)
    n_gas, n_layers, n_pts = a.shape
    if n_gas != los.n_gas:
        raise ValueError("%d coefficient sets for %d gases" % (n_gas, los.n_gas))
    da = de = jl = jp = rad = None
    if dcoeffs is not None:
        da, de = _gas_stack(dcoeffs)
        assert da.shape == a.shape
        jl = torch.empty((los.n_rays, n_layers if seg_jac_row is None else int(n_jac_rows), n_pts), dtype=torch.float64,
                         device="cuda")
    n_par, pg, pw = 0, None, None
    sjr, sjp = (None, None) if seg_jac_row is None else _i(seg_jac_row)
    if sjr is not None and sjr.size != los.n_seg:
        raise ValueError("seg_jac_row must be [n_seg]")
    if par_gas is not None:
        par_gas, pg = _i(par_gas)
        par_w, pw = _d(par_w)
        n_par = par_gas.size
        if par_w.shape != (n_par, los.n_pt):
            raise ValueError("par_w must be [n_par, n_pt]")
        jp = torch.empty((los.n_rays, n_par, n_pts), dtype=torch.float64, device="cuda")
    if want_rad:
        rad = torch.empty((los.n_rays, n_pts), dtype=torch.float64, device="cuda")
    d = los.desc(grid, g_lo)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    check(lib.sr_limb_rays_jacobians_dev(ptr(a), ptr(e), ptr(da), ptr(de), n_layers, n_pts, C.byref(d), sjp,
                                         0 if sjr is None else int(n_jac_rows), n_par, pg, pw, ptr(rad), ptr(jl), ptr(jp),
                                         _stream_ptr()), "sr_limb_rays_jacobians_dev")
    return rad, jl, jp


def _level_table_args(tab, coef_row, par_level, par_c, n_layers, n_pts, count):
    """(n_levels, n_tab_rows, coef_row pointer, number of level parameters, par_level pointer, par_c pointer): the
    level-table arguments of the two level Jacobians below, checked; `count` is what the caller's text calls the number."""
    assert tab.is_cuda and tab.dtype == torch.float64 and tab.is_contiguous() and tab.dim() == 4 and tab.shape[1] == 2
    if tab.shape[3] != n_pts:
        raise ValueError("tables of %d points for coefficients of %d" % (tab.shape[3], n_pts))
    coef_row, cr = _i(coef_row)
    par_level, pl = _i(np.asarray(par_level).reshape(-1))
    par_c, pc = _d(par_c)
    if coef_row.shape != (n_layers,):
        raise ValueError("coef_row must be [n_layers]")
    if par_c.shape != (par_level.size, n_layers):
        raise ValueError("par_c must be [%s, n_layers]" % count)
    return int(tab.shape[0]), int(tab.shape[2]), cr, par_level.size, pl, pc


def limb_rays_level_jacobian(coeffs, los, tab, coef_row, par_level, par_c, gas=0, grid=None, g_lo=0, want_rad=True):
    """(rad | None, jac [n_rays, n_par, n_pts]): radiances and their derivatives with respect to level parameters of
    the level-factored gas `gas` (sr_limb_rays_jac_level_dev).  coeffs as limb_rays; tab: that gas's pair tables (CUDA
    [n_levels, 2, n_tab_rows, n_pts], LineSet.glevel_pairs); coef_row [n_layers]: the table row of every coefficient
    row; parameter p moves the population of level par_level[p] on coefficient row r by par_c[p, r].  Vibrational
    temperatures: LevelFactored.tvib_jacobian."""
    a, e = _gas_stack(coeffs)
    n_gas, n_layers, n_pts = a.shape
    if n_gas != los.n_gas:
        raise ValueError("%d coefficient sets for %d gases" % (n_gas, los.n_gas))
    n_levels, n_tab_rows, cr, n_par, pl, pc = _level_table_args(tab, coef_row, par_level, par_c, n_layers, n_pts, "n_par")
    rad = torch.empty((los.n_rays, n_pts), dtype=torch.float64, device="cuda") if want_rad else None
    jac = torch.empty((los.n_rays, n_par, n_pts), dtype=torch.float64, device="cuda")
    d = los.desc(grid, g_lo)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    check(lib.sr_limb_rays_jac_level_dev(ptr(a), ptr(e), n_layers, n_pts, C.byref(d), int(gas), ptr(tab), n_levels, n_tab_rows,
                                         cr, n_par, pl, pc, ptr(rad), ptr(jac), _stream_ptr()),
          "sr_limb_rays_jac_level_dev")
    return rad, jac


def limb_rays_state_jacobian(coeffs, los, par_gas=None, par_w=None, tab=None, coef_row=None, par_level=None, par_c=None,
                             gas=0, grid=None, g_lo=0, want_rad=True, dcoeffs=None, par_t=None, level_gases=None, par_lgas=None,
                             pointing=False, ray_blocks=None):
    """(rad | None, jac [n_rays, n_col + n_lev (+ n_row), n_pts]): radiances and their derivatives with respect to a
    mixed state vector in ONE pass over each ray (sr_limb_rays_jac_state_dev): the column parameters par_gas / par_w of
    limb_rays_jacobian (VMR-profile parameters, par_w [n_col, n_pt] at the LOS sample points) first, then the level
    parameters tab / coef_row / par_level / par_c of limb_rays_level_jacobian for the level-factored gas `gas`
    (par_c [n_lev, n_layers] on the coefficient rows).  Either kind may be left out (None), not both.  Vibrational
    temperatures: LevelFactored.state_jacobian.
    dcoeffs and par_t (both or neither) add ROW parameters as a third kind, behind the other two
    (sr_limb_rays_jac_state_rows_dev): dcoeffs stacks like coeffs, the derivatives of every gas's (abs, emi) with respect
    to one scalar per coefficient row (kinetic temperature: coefficients_dT, LevelFactored.steps(derivative=True)), and
    row parameter p moves that scalar on row r by par_t[p, r] (par_t [n_row, n_layers], node masks).  It is
    limb_rays_layer_jacobian contracted with par_t inside the recursion.  The columns are held fixed, as in
    temperature_jacobian; the density part of a temperature change is a set of column parameters, which the caller adds
    to par_gas / par_w if it is wanted.  With row parameters the other two kinds may both be left out.
    level_gases and par_lgas (both or neither; then without tab / coef_row / gas): the level parameters of SEVERAL
    level-factored gases in the same pass (sr_limb_rays_jac_state_gases_dev): level_gases = [(gas, tab, coef_row), ...],
    one entry per level-factored gas of the batch (its index there, its pair tables, its row map; tables may differ in
    levels and rows), and level parameter p belongs to level_gases[par_lgas[p]], to its level par_level[p].  The rows of
    jac keep the caller's order.  Vibrational temperatures: LevelFactoredSet.state_jacobian.
    pointing=True (sr_limb_rays_jac_state_path_dev; the batch needs path=, else ValueError): one more row behind the
    state's, jac [n_rays, n_par + 1, n_pts] (a view), d rad / d z_t of every ray's own tangent altitude [per km] with the
    crossed shells held fixed; the other rows and rad are those of the call without, bit for bit, and there may be no
    other parameter.  Limb rays of geometry.limb_los only: 3-D paths, slant / nadir paths, adaptive stepping, observer
    order, the resident-handle routes and refraction are not supported.
    ray_blocks (None: as set_state_ray_blocks left it): parameter blocks per ray, or the dense plan, for this call."""
    with _RayBlocks(ray_blocks):
        return _limb_rays_state_jacobian(coeffs, los, par_gas, par_w, tab, coef_row, par_level, par_c, gas, grid, g_lo, want_rad,
                                         dcoeffs, par_t, level_gases, par_lgas, pointing)


def _limb_rays_state_jacobian(coeffs, los, par_gas, par_w, tab, coef_row, par_level, par_c, gas, grid, g_lo, want_rad, dcoeffs,
                              par_t, level_gases, par_lgas, pointing):
    if pointing:
        path = los.path_desc()
    A = _state_args(coeffs, los, par_gas, par_w, tab, coef_row, par_level, par_c, gas, grid, g_lo, dcoeffs, par_t, level_gases,
                    par_lgas, may_be_empty=bool(pointing), as_list=bool(pointing))
    n_pts = A.a.shape[2]
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    rad = torch.empty((los.n_rays, n_pts), dtype=torch.float64, device="cuda") if want_rad else None
    if pointing:
        jac = torch.empty((los.n_rays, A.n_par + los.n_gas, n_pts), dtype=torch.float64, device="cuda")
        name = "sr_limb_rays_jac_state_path_dev"
        check(getattr(lib, name)(*A.args(name, C.byref(path), ptr(rad), ptr(jac), _stream_ptr())), name)
        return rad, jac[:, :A.n_par + 1]
    jac = torch.empty((los.n_rays, A.n_par, n_pts), dtype=torch.float64, device="cuda")
    name = _state_entry(False, False, level_gases is not None, par_t is not None)
    check(getattr(lib, name)(*A.args(name, ptr(rad), ptr(jac), _stream_ptr())), name)
    return rad, jac


def _state_entry(bands, instrument, several, rows):
    """The library entry of a mixed-state call: spectra or the instrument's bands, those with the instrument rows, the
    level parameters of one level-factored gas or of a list of them; the spectra of one gas with or without row parameters
    (the bands entries take both)."""
    if bands:
        return "sr_limb_rays_state_bands%s%s_dev" % ("_instr" if instrument else "", "_gases" if several else "")
    return "sr_limb_rays_jac_state%s_dev" % ("_gases" if several else "_rows" if rows else "")


class _StateArgs(object):
    """What _state_args returns: a, e (the stacked coefficients), desc, n_col, n_lev, n_row, n_par, args(entry, *tail) --
    the argument tuple of the named mixed-state entry, `tail` behind the parameters' (outputs or bands, stream) -- and
    keep, the arrays and tensors its pointers point into."""

    def args(self, entry, *tail):
        batch, levels, rows = self._blocks
        if entry == "sr_limb_rays_jac_state_dev":   # the one entry without row parameters
            rows = ()
        return batch + levels + rows + tail


def _level_gases_args(level_gases, par_lgas, tab, coef_row, par_level, par_c, n_gas, n_layers, n_pts):
    """The list of level gases of a mixed-state call, checked and marshalled: (LevelGasDesc array, n_lgas, n_lev, pointers to
    par_lgas, par_level, par_c, what they point into)."""
    if par_lgas is None:
        raise ValueError("level_gases needs par_lgas, the level gas of every level parameter")
    if tab is not None or coef_row is not None:
        raise ValueError("level_gases carries the tables and row maps: give no tab / coef_row beside it")
    level_gases = list(level_gases)
    if not 1 <= len(level_gases) <= min(n_gas, LevelFactoredSet.MAX_MEMBERS):
        raise ValueError("%d level gases for a batch of %d gases (at most %d are level-factored)"
                         % (len(level_gases), n_gas, LevelFactoredSet.MAX_MEMBERS))
    arr, keep, seen = (_lib.LevelGasDesc * len(level_gases))(), [], set()
    for k, (g, t, cr) in enumerate(level_gases):
        g = int(g)
        if not 0 <= g < n_gas or g in seen:
            raise ValueError("level gas %d: gas %d is out of range or named twice" % (k, g))
        seen.add(g)
        if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.dim() == 4 and t.shape[1] == 2):
            raise ValueError("level gas %d: its tables must be a contiguous CUDA float64 [n_levels, 2, n_tab_rows, n_pts]" % k)
        if t.shape[3] != n_pts:
            raise ValueError("tables of %d points for coefficients of %d" % (t.shape[3], n_pts))
        cr, crp = _i(cr)
        if cr.shape != (n_layers,):
            raise ValueError("coef_row must be [n_layers]")
        arr[k].gas, arr[k].n_levels, arr[k].n_tab_rows = g, int(t.shape[0]), int(t.shape[2])
        arr[k].tab, arr[k].coef_row = t.data_ptr(), crp
        keep.append((t, cr))
    par_level, pl = _i(np.asarray([] if par_level is None else par_level).reshape(-1))
    par_lgas, plg = _i(np.asarray(par_lgas).reshape(-1))
    if par_lgas.size != par_level.size:
        raise ValueError("par_lgas must be [n_lev], one level gas per level parameter")
    if par_lgas.size and (par_lgas.min() < 0 or par_lgas.max() >= len(level_gases)):
        raise ValueError("par_lgas out of range")
    pc = None
    if par_level.size:
        if par_c is None:
            raise ValueError("level parameters need par_c")
        par_c, pc = _d(par_c)
        if par_c.shape != (par_level.size, n_layers):
            raise ValueError("par_c must be [n_lev, n_layers]")
        n_lv = np.array([a.n_levels for a in arr])[par_lgas]
        if par_level.min() < 0 or np.any(par_level >= n_lv):
            raise ValueError("par_level out of range for its level gas")
    return arr, len(level_gases), par_level.size, plg, pl, pc, (keep, par_lgas, par_level, par_c)


def _state_args(coeffs, los, par_gas, par_w, tab, coef_row, par_level, par_c, gas, grid, g_lo, dcoeffs, par_t, level_gases=None,
                par_lgas=None, may_be_empty=False, as_list=False):
    """The arguments of a mixed-state call (limb_rays_state_jacobian, limb_rays_state_bands), checked and marshalled: the
    one place where their shapes are refused.  may_be_empty: a call that returns something without any parameter (the
    bands call with its instrument rows, the calls with the pointing row).  as_list: the one level gas of tab / coef_row
    / gas as a list of one (the entries with the pointing row take the list form only)."""
    if (dcoeffs is None) != (par_t is None):
        raise ValueError("row parameters need both dcoeffs and par_t")
    a, e = _gas_stack(coeffs)
    n_gas, n_layers, n_pts = a.shape
    if n_gas != los.n_gas:
        raise ValueError("%d coefficient sets for %d gases" % (n_gas, los.n_gas))
    n_col = n_lev = n_row = n_levels = n_tab_rows = 0
    pg = pw = cr = pl = pc = pt = da = de = None
    if par_gas is not None and np.asarray(par_gas).size:
        par_gas, pg = _i(np.asarray(par_gas).reshape(-1))
        par_w, pw = _d(par_w)
        n_col = par_gas.size
        if par_w.shape != (n_col, los.n_pt):
            raise ValueError("par_w must be [n_col, n_pt]")
    several = None
    if level_gases is not None:
        several = _level_gases_args(level_gases, par_lgas, tab, coef_row, par_level, par_c, n_gas, n_layers, n_pts)
        n_lev = several[2]
    elif par_lgas is not None:
        raise ValueError("par_lgas belongs to level_gases")
    elif par_level is not None and np.asarray(par_level).size:
        if tab is None or coef_row is None or par_c is None:
            raise ValueError("level parameters need tab, coef_row and par_c")
        n_levels, n_tab_rows, cr, n_lev, pl, pc = _level_table_args(tab, coef_row, par_level, par_c, n_layers, n_pts, "n_lev")
    d = los.desc(grid, g_lo)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    if par_t is not None:
        da, de = _gas_stack(dcoeffs)
        if da.shape != a.shape:
            raise ValueError("dcoeffs must stack to the shape of coeffs, [%d, %d, %d]" % tuple(a.shape))
        par_t, pt = _d(par_t)
        if par_t.ndim != 2 or par_t.shape[1] != n_layers:
            raise ValueError("par_t must be [n_row, n_layers]")
        n_row = par_t.shape[0]
        if n_col + n_lev + n_row == 0 and not may_be_empty:
            raise ValueError("no parameters: give column parameters, level parameters or row parameters")
    elif n_col + n_lev == 0 and not may_be_empty:
        raise ValueError("no parameters: give column parameters, level parameters or both")
    A = _StateArgs()
    A.a, A.e, A.desc, A.n_col, A.n_lev, A.n_row, A.n_par = a, e, d, n_col, n_lev, n_row, n_col + n_lev + n_row
    A.keep = (par_gas, par_w, tab, cr, pl, pc, da, de, par_t)
    levels = (int(gas), ptr(tab) if n_lev else None, n_levels, n_tab_rows, cr, n_lev, pl, pc)
    if several is not None:   # (the entries for a list of level gases)
        arr, n_lgas, _, plg, pl, pc, keep = several
        A.keep = A.keep + (arr, keep)
        levels = (n_lgas, arr, n_lev, plg, pl, pc)
    elif as_list:
        arr = (_lib.LevelGasDesc * 1)()
        arr[0].gas, arr[0].n_levels, arr[0].n_tab_rows = int(gas), n_levels, n_tab_rows
        arr[0].tab, arr[0].coef_row = (tab.data_ptr() if n_lev else None), cr
        A.keep = A.keep + (arr,)
        levels = (1, arr, n_lev, None, pl, pc)
    A._blocks = ((ptr(a), ptr(e), n_layers, n_pts, C.byref(d), n_col, pg, pw), levels, (ptr(da), ptr(de), n_row, pt))
    return A


def limb_rays_state_bands(coeffs, los, grid, centers_nm, widths_nm, par_gas=None, par_w=None, tab=None, coef_row=None,
                          par_level=None, par_c=None, gas=0, dcoeffs=None, par_t=None, out_units="Wm2", n_sigma=5.0, fov=None,
                          g_lo=0, level_gases=None, par_lgas=None, instrument=False, pointing=False, ils=None, ray_blocks=None):
    """limb_rays_state_jacobian on the instrument's bands in ONE library call (sr_limb_rays_state_bands_dev): the same
    mixed state vector (column, level, row parameters: the same arguments, the same errors), but no hi-res spectrum is
    written -- the recursion kernel integrates the bands in its epilogue.  Returns numpy [n_rays | n_rays / 3, 1 + n_par,
    n_bands] in out_units: row 0 the radiance, row 1 + p its derivative to parameter p (column, level, row parameters, each
    kind in the caller's order).  What limb_rays_state_jacobian + hires_to_lowres on rad and jac (+ fov_closed_form) give,
    up to the order of the band sums.  fov: fov_factors of the pixels, three rays each.  A spectral shard (g_lo, the
    coefficient tables' width; `grid` is always the whole grid) gives its partial band integrals, as hires_to_lowres.
    level_gases / par_lgas: several level-factored gases, as in limb_rays_state_jacobian
    (sr_limb_rays_state_bands_gases_dev).
    instrument=True (sr_limb_rays_state_bands_instr[_gases]_dev): two more rows behind the parameters', [.., 1 + n_par + 2,
    n_bands]: the derivatives of the radiance's bands to the band centre (per nm) and to the logarithm of the ILS width, as
    hires_to_lowres_instrument defines them (window membership held fixed); rows 0 .. n_par are those of the call without
    them, bit for bit, and there may then be no parameter at all.
    pointing=True (sr_limb_rays_state_bands_path_dev; the batch needs path=, else ValueError): the pointing row of
    limb_rays_state_jacobian behind the parameters' and in front of the instrument rows, [.., 1 + n_par + 1 (+ 2),
    n_bands]; the other rows are those of the call without, bit for bit.
    ils: an ILS, the bands' tabulated line shape (as hires_to_lowres and, with instrument=True, hires_to_lowres_instrument).
    ray_blocks (None: as set_state_ray_blocks left it): parameter blocks per ray, or the dense plan, for this call."""
    with _RayBlocks(ray_blocks):
        return _limb_rays_state_bands(coeffs, los, grid, centers_nm, widths_nm, par_gas, par_w, tab, coef_row, par_level, par_c, gas,
                                      dcoeffs, par_t, out_units, n_sigma, fov, g_lo, level_gases, par_lgas, instrument, pointing, ils)


def _limb_rays_state_bands(coeffs, los, grid, centers_nm, widths_nm, par_gas, par_w, tab, coef_row, par_level, par_c, gas, dcoeffs,
                           par_t, out_units, n_sigma, fov, g_lo, level_gases, par_lgas, instrument, pointing, ils):
    instrument, pointing = bool(instrument), bool(pointing)
    if pointing:
        path = los.path_desc()
    A = _state_args(coeffs, los, par_gas, par_w, tab, coef_row, par_level, par_c, gas, grid, g_lo, dcoeffs, par_t, level_gases,
                    par_lgas, may_be_empty=instrument or pointing, as_list=pointing)
    n_pts = A.a.shape[2]
    w0, step, n = grid_params(grid)
    A.desc.w0, A.desc.step = w0, step   # (the grid of the bands; with a Planck background desc() has set the same)
    centers_nm, cp = _d(centers_nm)
    widths_nm, wp = _d(widths_nm)
    if widths_nm.size != centers_nm.size:
        raise ValueError("{} spectral widths for {} grid points".format(widths_nm.size, centers_nm.size))
    if not (0 <= g_lo and g_lo + n_pts <= n):
        raise ValueError("the coefficient tables cover grid points outside the grid")
    n_out, fp = los.n_rays, None
    if fov is not None:
        fov, fp = _d(fov)
        if los.n_rays % 3 or fov.shape != (los.n_rays // 3, 7):
            raise ValueError("fov must be [n_rays / 3, 7] (three rays per pixel)")
        n_out = los.n_rays // 3
    out = np.empty((n_out, 1 + A.n_par + (1 if pointing else 0) + (2 if instrument else 0), centers_nm.size))
    if pointing:
        name = "sr_limb_rays_state_bands_path_dev"
        with _IlsBound(ils):
            check(getattr(lib, name)(*A.args(name, cp, wp, centers_nm.size, float(n_sigma), _UNITS[out_units], fp,
                                             out.ctypes.data_as(dp), _stream_ptr(), int(instrument), C.byref(path))), name)
        return out
    name = _state_entry(True, instrument, level_gases is not None, par_t is not None)
    with _IlsBound(ils):
        check(getattr(lib, name)(*A.args(name, cp, wp, centers_nm.size, float(n_sigma), _UNITS[out_units], fp,
                                         out.ctypes.data_as(dp), _stream_ptr())), name)
    return out


def limb_rays_parts(coeffs, los, part_gas, part_level, part_c=None, tab=None, coef_row=None, gas=0, grid=None, g_lo=0,
                    want_rad=True):
    """(rad | None, parts [n_rays, n_part + 1, n_pts]): the radiances split into the parts single gases and single levels
    emit (sr_limb_rays_parts_dev): part k is the radiance that arrives from a share of one gas's emission, attenuated by
    ALL gases.  part_level[k] = -1: the whole emission of gas part_gas[k]; >= 0: level part_level[k] of the
    level-factored gas `gas` (part_gas[k] must be gas), its share on coefficient row r being part_c[k, r] *
    tab[level, 1, coef_row[r]] -- part_c the level's populations, or populations times an altitude mask.  The last row of
    `parts` is the background (the initial intensity, attenuated); the gas parts and the background add up to rad.
    coeffs as limb_rays; tab: the gas's pair tables (CUDA [n_levels, 2, n_tab_rows, n_pts], LineSet.glevel_pairs);
    coef_row [n_layers]; part_c [n_part, n_layers] (rows of gas parts ignored); the three are needed for level parts
    only.  Populations of a gas's levels: LevelFactored.level_radiances."""
    _four_gas_call("limb_rays_parts", los)
    a, e = _gas_stack(coeffs)
    n_gas, n_layers, n_pts = a.shape
    if n_gas != los.n_gas:
        raise ValueError("%d coefficient sets for %d gases" % (n_gas, los.n_gas))
    part_gas, pg = _i(np.asarray(part_gas).reshape(-1))
    part_level, pl = _i(np.asarray(part_level).reshape(-1))
    n_part = part_level.size
    if part_gas.size != n_part:
        raise ValueError("part_gas and part_level must have the same length")
    n_levels = n_tab_rows = 0
    cr = pc = None
    if n_part and part_level.max() >= 0:
        if tab is None or coef_row is None or part_c is None:
            raise ValueError("level parts need tab, coef_row and part_c")
    if tab is not None:
        assert tab.is_cuda and tab.dtype == torch.float64 and tab.is_contiguous() and tab.dim() == 4 and tab.shape[1] == 2
        if tab.shape[3] != n_pts:
            raise ValueError("tables of %d points for coefficients of %d" % (tab.shape[3], n_pts))
        n_levels, n_tab_rows = int(tab.shape[0]), int(tab.shape[2])
    if coef_row is not None:
        coef_row, cr = _i(coef_row)
        if coef_row.shape != (n_layers,):
            raise ValueError("coef_row must be [n_layers]")
    if part_c is not None:
        part_c, pc = _d(part_c)
        if part_c.shape != (n_part, n_layers):
            raise ValueError("part_c must be [n_part, n_layers]")
    rad = torch.empty((los.n_rays, n_pts), dtype=torch.float64, device="cuda") if want_rad else None
    parts = torch.empty((los.n_rays, n_part + 1, n_pts), dtype=torch.float64, device="cuda")
    d = los.desc(grid, g_lo)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    check(lib.sr_limb_rays_parts_dev(ptr(a), ptr(e), n_layers, n_pts, C.byref(d), int(gas), ptr(tab), n_levels, n_tab_rows,
                                     cr, n_part, pg, pl, pc, ptr(rad), ptr(parts), _stream_ptr()), "sr_limb_rays_parts_dev")
    return rad, parts


def radiance_jacobian(abs_c, emi_c, seg_off, seg_layer, seg_col, dcol_dpar):
    """Radiances [n_rays, n_pts] and d rad / d x_p [n_rays, n_par, n_pts] for parameters on which the
    segment columns depend linearly: dcol_dpar[s, p] = d col_s / d x_p (sr_radiance_jac_dev)."""
    assert abs_c.is_cuda and abs_c.dtype == torch.float64 and abs_c.is_contiguous()
    assert emi_c.shape == abs_c.shape and emi_c.is_contiguous()
    n_layers, n_pts = abs_c.shape
    seg_off, op = _i(seg_off)
    seg_layer, lp = _i(seg_layer)
    seg_col, cp = _d(seg_col)
    dcol, dpp = _d(dcol_dpar)
    if dcol.ndim != 2 or dcol.shape[0] != seg_col.size:
        raise ValueError("dcol_dpar must be [n_seg, n_par]")
    n_rays, n_par = seg_off.size - 1, dcol.shape[1]
    rad = torch.empty((n_rays, n_pts), dtype=torch.float64, device="cuda")
    jac = torch.empty((n_rays, n_par, n_pts), dtype=torch.float64, device="cuda")
    check(lib.sr_radiance_jac_dev(C.c_void_p(abs_c.data_ptr()), C.c_void_p(emi_c.data_ptr()), n_layers, n_pts,
                                  n_rays, op, lp, cp, dpp, n_par, C.c_void_p(rad.data_ptr()),
                                  C.c_void_p(jac.data_ptr()), _stream_ptr()), "sr_radiance_jac_dev")
    return rad, jac


def radiance_layer_jacobian(abs_c, emi_c, dabs, demi, seg_off, seg_layer, seg_col):
    """d rad / d (one scalar per layer) [n_rays, n_layers, n_pts], the scalar acting through the layer's own
    coefficients: dabs, demi [n_layers, n_pts] = d(abs, emi of layer k)/d(parameter of layer k)
    (sr_radiance_jac_layer_dev)."""
    for t in (abs_c, emi_c, dabs, demi):
        assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.shape == abs_c.shape
    n_layers, n_pts = abs_c.shape
    seg_off, op = _i(seg_off)
    seg_layer, lp = _i(seg_layer)
    seg_col, cp = _d(seg_col)
    n_rays = seg_off.size - 1
    jac = torch.empty((n_rays, n_layers, n_pts), dtype=torch.float64, device="cuda")
    check(lib.sr_radiance_jac_layer_dev(C.c_void_p(abs_c.data_ptr()), C.c_void_p(emi_c.data_ptr()),
                                        C.c_void_p(dabs.data_ptr()), C.c_void_p(demi.data_ptr()), n_layers, n_pts,
                                        n_rays, op, lp, cp, C.c_void_p(jac.data_ptr()), _stream_ptr()),
          "sr_radiance_jac_layer_dev")
    return jac


def calc_radtran_steps(gases, z, temps, press, z_tans, radtran_opt=None, R=2575.0, n_sub=3, **los_opts):
    """Adaptive LOS stepping + the coefficient rows of the steps, with the reference's knobs: radtran_opt =
    dict(max_T_variation=[K], max_Plog_variation=[ln P], max_opt_depth=...) as its drivers pass them to
    LineOfSight.calc_radtran_steps (spect_main_module.py:2746-2767; radtran_test_CO.py:184-186;
    spect_radtran_test.py:175).  gases: [dict(lineset=LineSet, vmr=[n_levels], iso_ratio=1.0, tvib=[n_lev, n_levels] | None)].
    Geometry by geometry.calc_radtran_steps (temperature / log-pressure bounds, vectorised); the optical-depth bound is
    checked on the device: the steps' coefficient rows at their own (P, T) -- abscoeff_layers on the step list --, per
    step the largest absorption coefficient over the grid times the step's Curtis-Godson column (sr_los_columns),
    summed over the gases; steps above the bound are halved and only then re-evaluated.
    Returns dict(L=geometry dict, los=LimbLOS, coeffs=[(abs, emi)] per gas on the step rows [n_steps, n_grid])."""
    from . import geometry as geo, synthetic as syn
    opt = dict(radtran_opt or {})
    z, temps, press = (np.asarray(v, float) for v in (z, temps, press))
    nd = syn.number_density(press, temps)
    vm = [np.asarray(g["vmr"], float) for g in gases]
    state = {}

    def rows(L):
        key = (len(L["step_temp"]), float(L["step_temp"].sum()), float(L["x"].sum()))
        if state.get("key") != key:
            co = []
            for g in gases:
                tv = None
                if g.get("tvib") is not None:     # vibrational temperatures linear in altitude between the levels, like T
                    tvl = np.asarray(g["tvib"], float)
                    zz = np.append(z, z[-1] + (z[-1] - z[-2]))
                    tv = np.array([np.interp(L["step_alt"], zz, np.append(t, t[-1])) for t in tvl])
                co.append(g["lineset"].abscoeff_layers(L["step_temp"], L["step_pres"], tvib=tv))
            los = LimbLOS(L["seg_off"], L["seg_layer"], L["pt_off"], L["x"], L["nd"], L["vmr"],
                          col_scale=[g.get("iso_ratio", 1.0) for g in gases], **los_opts)
            state.update(key=key, coeffs=co, los=los)
        return state["coeffs"], state["los"]

    def opt_depth_of(L):
        co, los = rows(L)
        col = los.columns()                                   # [n_gas, n_steps]
        amax = np.array([c[0].abs().amax(dim=1).cpu().numpy() for c in co])
        return (amax * col).sum(axis=0)

    L = geo.calc_radtran_steps(z, temps, press, nd, vm, z_tans, R=R, n_sub=n_sub,
                               max_T_variation=opt.get("max_T_variation"), max_Plog_variation=opt.get("max_Plog_variation"),
                               max_opt_depth=opt.get("max_opt_depth"), opt_depth_of=opt_depth_of if opt.get("max_opt_depth") else None)
    co, los = rows(L)
    return dict(L=L, los=los, coeffs=co)


def mix_gases(coeffs, ratios):
    """Coefficients of a gas mixture on the column scale of a reference absorber: the column of gas g in
    a segment of layer k is ratios[g][k] times the reference column (VMR_g / VMR_ref of the layer), so
    tau = (sum_g ratios[g][k] abs_g[k]) * u_ref.  coeffs: [(abs_g, emi_g)] CUDA [n_layers, n_pts] on one
    grid; ratios: [n_gas][n_layers].  Returns (abs_mix, emi_mix)."""
    a_mix = e_mix = None
    for (a, e), r in zip(coeffs, ratios):
        w = torch.as_tensor(np.ascontiguousarray(r, dtype=np.float64), device=a.device)[:, None]
        a_mix = a * w if a_mix is None else a_mix + a * w
        e_mix = e * w if e_mix is None else e_mix + e * w
    return a_mix.contiguous(), e_mix.contiguous()


def gas_layer_jacobian(abs_mix, emi_mix, abs_g, emi_g, dratio_dx, seg_off, seg_layer, seg_col):
    """d rad / d x_k [n_rays, n_layers, n_pts] for one scalar per layer that scales gas g's amount in
    that layer inside a mixture (its VMR): the mixture's coefficients depend on it through
    d abs_mix[k]/d x_k = dratio_dx[k] * abs_g[k] (same for emi), which is the layer Jacobian's input.
    Profile parameters follow by the chain rule: J_p = sum_k mask_p[k] * J_k."""
    w = torch.as_tensor(np.ascontiguousarray(dratio_dx, dtype=np.float64), device=abs_g.device)[:, None]
    return radiance_layer_jacobian(abs_mix, emi_mix, (abs_g * w).contiguous(), (emi_g * w).contiguous(),
                                   seg_off, seg_layer, seg_col)


def coefficients_dT(ls, temps, press, tvib=None, q_part=None, g_lo=0, g_hi=None, scheme="central", dT=None,
                    coeffs=None, frozen=True):
    """(abs, emi) at T and their derivatives with respect to each layer's kinetic temperature (pressure and, in
    non-LTE, the vibrational temperatures held fixed; with q_part=None the partition sum follows T).  The reference
    has no temperature Jacobian (spect_main_module.py:300-306 is commented out): build's definition, by finite
    differences of the coefficient op.

    frozen (default): the perturbed ops place their Humlicek region boundaries as at T (LineSet.set_bounds_temps).
    The regions disagree by 1e-5..1e-4 at their index-computed seams; with boundaries that move with T a difference
    quotient carries a spike of (1e-5 y) / dT wherever a seam crosses a point.  What remains non-smooth in T is the
    reference's single-precision cmplx(ry, -rx) (lineshape.f:529): a staircase of ~1e-7 of a core value, i.e. noise of
    ~1e-7 |c| / dT in any quotient -- which is what bounds dT from below.
      scheme "central" (default, THREE coefficient ops): (c(T + dT) - c(T - dT)) / 2 dT, dT = 0.05 K: ~3e-5 of a
        layer's largest derivative (2e-4 with moving boundaries, frozen=False: rounds 1-3's definition).
      scheme "forward" (TWO ops): (c(T + dT) - c(T)) / dT, dT = 0.002 K: ~3e-4, and 1.5e-3 for the emission coefficient
        of a Doppler layer (truncation dT/2 |c''|, with c'' / c' up to 0.3 / K from level populations and Doppler
        cores, against the staircase noise): good for a Gauss-Newton step, a third cheaper.
    tests/test_gpu_configs.py::test_temperature_derivative_schemes measures the three against each other;
    tests/test_frozen_reference_host.py measures the frozen two against a smooth, extrapolated derivative of the CPU
    reference (central 1.1e-5 abs | 2.5e-5 emi, forward 3.4e-4 | 1.5e-3 at the worst of four layers, 1e-3 to 1013 hPa)."""
    temps = np.ascontiguousarray(temps, dtype=np.float64)
    kw = dict(tvib=tvib, q_part=q_part, g_lo=g_lo, g_hi=g_hi)
    if scheme not in ("forward", "central"):
        raise ValueError("scheme must be 'forward' or 'central'")
    if coeffs is None:
        coeffs = ls.abscoeff_layers(temps, press, **kw)
    if frozen:
        ls.set_bounds_temps(temps)
    try:
        if scheme == "forward":
            dT = 0.002 if dT is None else dT
            a_p, e_p = ls.abscoeff_layers(temps + dT, press, **kw)
            return coeffs, ((a_p - coeffs[0]) / dT, (e_p - coeffs[1]) / dT)
        dT = 0.05 if dT is None else dT
        a_p, e_p = ls.abscoeff_layers(temps + dT, press, **kw)
        a_m, e_m = ls.abscoeff_layers(temps - dT, press, **kw)
        return coeffs, ((a_p - a_m) / (2.0 * dT), (e_p - e_m) / (2.0 * dT))
    finally:
        if frozen:
            ls.set_bounds_temps(None)


def temperature_jacobian(ls, temps, press, seg_off, seg_layer, seg_col, tvib=None, q_part=None, dT=0.05,
                         g_lo=0, g_hi=None, coeffs=None):
    """d rad / d T_k [n_rays, n_layers, n_pts] for the kinetic temperature of every layer (pressure,
    columns and, in non-LTE, the vibrational temperatures held fixed): the coefficient op at T + dT
    and T - dT (coefficients_dT: central differences of the layer's own abs / emi with the region boundaries
    frozen at T; with q_part=None the partition sum follows T), then the forward sensitivity of the radiance
    recursion.  `coeffs` = (abs, emi) at T
    if already computed.  The reference has no temperature Jacobian: build's definition."""
    coeffs, (dabs, demi) = coefficients_dT(ls, temps, press, tvib=tvib, q_part=q_part, g_lo=g_lo, g_hi=g_hi,
                                           scheme="central", dT=dT, coeffs=coeffs)
    return radiance_layer_jacobian(coeffs[0], coeffs[1], dabs, demi, seg_off, seg_layer, seg_col)


def set_points_per_lane(p):
    check(lib.sr_set_points_per_lane(int(p)), "sr_set_points_per_lane")


def set_level_route(multi_channel):
    """1 (default): level tables (glevel_pairs, gcoeff_levels) by the multi-channel pass -- every line once --; 0: one
    coefficient op per level (sr_set_level_route)."""
    check(lib.sr_set_level_route(int(multi_channel)), "sr_set_level_route")


def set_overlap(on):
    """1 (default): the zones kernel runs beside the far-field kernel on an internal stream;
    0: kernels one after the other (per-kernel times in last_kernel_ms)."""
    check(lib.sr_set_overlap(int(on)), "sr_set_overlap")


def far_field_truncation_bound():
    """18 theta^-(degree + 1): what the far-field mode may differ by from the exact mode, relative to a line's own
    contribution (sr_far_field_truncation_bound; 1.6e-11 as built by default)."""
    return float(lib.sr_far_field_truncation_bound())


def far_field_min_distance(level, pole_margin):
    """Grid points between a level-`level` box's centre and a line's centre index from which the box takes the line by
    its expansion, as the kernels decide it (sr_far_field_min_distance); pole_margin: the layer's, in grid points."""
    d = float(lib.sr_far_field_min_distance(int(level), int(pole_margin)))
    if d < 0.0:
        raise ValueError("far_field_min_distance: level in [0, 5) and pole_margin >= 0")
    return d


def far_field_degree(theta=4):
    """The expansion degree the library was built with (from its truncation bound 18 theta^-(degree + 1))."""
    import math
    return int(round(math.log(18.0 / far_field_truncation_bound()) / math.log(theta))) - 1


def set_band_fusion(on):
    """1 (default): a retrieval iteration's recursion kernel integrates the instrument bands itself; 0: spectra, then the
    instrument step's own kernels (sr_set_band_fusion; the check and the A/B partner)."""
    check(lib.sr_set_band_fusion(int(bool(on))), "sr_set_band_fusion")


_state_ray_blocks = False  # what set_state_ray_blocks last set (the library's default: off)


def set_state_ray_blocks(on):
    """False (default): the mixed-state calls cut the parameter list of the batch into blocks and walk every ray once per
    block; True: every ray has its own list -- the parameters that touch it -- and is walked once per block of that list
    (sr_set_state_ray_blocks).  The rows of parameters that do not touch a ray are exact zeros either way.  For states
    whose parameters each act on few rays: latitude boxes, many altitude nodes."""
    global _state_ray_blocks
    check(lib.sr_set_state_ray_blocks(int(bool(on))), "sr_set_state_ray_blocks")
    _state_ray_blocks = bool(on)


class _RayBlocks(object):
    """The ray_blocks= keyword of the mixed-state calls: the switch for one call, then what it was (None: as it is)."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.was = _state_ray_blocks
        if self.on is not None:
            set_state_ray_blocks(self.on)

    def __exit__(self, *exc):
        if self.on is not None:
            set_state_ray_blocks(self.was)
        return False


def last_state_route():
    """(route, walks) of this thread's last mixed-state call: route 1 the dense plan, 2 parameter blocks per ray, 0 none
    yet; walks: its (ray, block) pairs, how often a ray was walked (sr_last_state_route, sr_last_state_walks)."""
    return int(lib.sr_last_state_route()), int(lib.sr_last_state_walks())


StateInstance = collections.namedtuple("StateInstance", "ng np cols rows bands instr several rayblk")


def last_state_instance():
    """StateInstance(ng, np, cols, rows, bands, instr, several, rayblk): the compile-time parameters of the state kernel's
    instance that the calling thread's most recent mixed-state call launched (sr_last_state_instance) -- the template's
    gas count (6 for a five-gas batch, 8 for seven), its slots per block, and the flags as bools -- recorded at the
    launch itself, not what the call asked for.  None before the thread's first launch."""
    out = (C.c_int32 * 8)()
    if lib.sr_last_state_instance(out) != _lib.SR_OK:
        return None
    return StateInstance(int(out[0]), int(out[1]), *(bool(v) for v in out[2:]))


def state_ray_plan(los, n_layers, par_gas=None, par_w=None, par_level=None, par_c=None, par_t=None, par_lgas=None, n_hid=0):
    """The per-ray plan of a mixed-state call on the host (sr_state_ray_plan; no GPU is touched): a dict with np, n_blocks
    (the largest block count of a ray), ray_blk_off [n_rays + 1], blk [n_rb, 2], col_row [n_rb, np], ent_off [n_rb,
    n_layers + 1], slot_par [n_rb, np] and the entries ent_slot, ent_level, ent_c.  los: a LimbLOS; the parameter arrays as
    limb_rays_state_jacobian takes them."""
    d = los.desc(rad0=True)
    d.init_mode = 0   # (the plan does not depend on the initial intensity)
    n_col = n_lev = n_row = 0
    pg = pw = plg = pl = pc = pt = None
    if par_gas is not None and np.asarray(par_gas).size:
        par_gas, pg = _i(np.asarray(par_gas).reshape(-1))
        par_w, pw = _d(par_w)
        n_col = par_gas.size
        if par_w.shape != (n_col, los.n_pt):
            raise ValueError("par_w must be [n_col, n_pt]")
    if par_level is not None and np.asarray(par_level).size:
        par_level, pl = _i(np.asarray(par_level).reshape(-1))
        par_c, pc = _d(par_c)
        n_lev = par_level.size
        if par_c.shape != (n_lev, n_layers):
            raise ValueError("par_c must be [n_lev, n_layers]")
        if par_lgas is not None:
            par_lgas, plg = _i(np.asarray(par_lgas).reshape(-1))
            if par_lgas.size != n_lev:
                raise ValueError("par_lgas must be [n_lev]")
    if par_t is not None:
        par_t, pt = _d(par_t)
        if par_t.ndim != 2 or par_t.shape[1] != n_layers:
            raise ValueError("par_t must be [n_row, n_layers]")
        n_row = par_t.shape[0]
    sizes = np.zeros(4, dtype=np.int32)
    head = (C.byref(d), int(n_layers), n_col, pg, pw, n_lev, plg, pl, pc, n_row, pt, int(n_hid), sizes.ctypes.data_as(ip))
    check(lib.sr_state_ray_plan(*(head + (None,) * 8)), "sr_state_ray_plan")
    n_p, n_blocks, n_rb, n_ent = (int(v) for v in sizes)
    P = dict(np=n_p, n_blocks=n_blocks,
             ray_blk_off=np.zeros(los.n_rays + 1, dtype=np.int32), blk=np.zeros((n_rb, 2), dtype=np.int32),
             col_row=np.zeros((n_rb, n_p), dtype=np.int32), ent_off=np.zeros((n_rb, n_layers + 1), dtype=np.int32),
             slot_par=np.zeros((n_rb, n_p), dtype=np.int32), ent_slot=np.zeros(n_ent, dtype=np.int32),
             ent_level=np.zeros(n_ent, dtype=np.int32), ent_c=np.zeros(n_ent))
    ints = tuple(P[k].ctypes.data_as(ip) for k in ("ray_blk_off", "blk", "col_row", "ent_off", "slot_par", "ent_slot", "ent_level"))
    check(lib.sr_state_ray_plan(*(head + ints + (P["ent_c"].ctypes.data_as(dp),))), "sr_state_ray_plan")
    return P


def set_jac_layer_mode(forward):
    """0 (default): Jacobians of the device LOS pipeline in one pass -- folded (a ray's two segments of a shell together,
    every value stored once) where the rays share their coefficient rows (1-D atmospheres), else in path order; 1: the
    forward-sensitivity kernels; 2: path order, one ray per thread, always; 3: path order, two rays per thread sharing
    a shell's loads (sr_set_jac_layer_mode)."""
    check(lib.sr_set_jac_layer_mode(int(forward)), "sr_set_jac_layer_mode")


def last_limb_route():
    """Which recursion kernel the last limb_rays call of this thread launched: 1 path order, 2 the folded sweep
    (sr_last_limb_route; diagnostic)."""
    return int(lib.sr_last_limb_route())


FAR_FIELD_DEFAULT = 3  # the library's default far-field mode (sr_set_far_field)


def set_far_field(on):
    """1: far wings by per-line local expansions; 2: by box pairs (multipole moments of the lines of a source
    box, translated to the local expansions of the well-separated target boxes); 3 (default): box pairs, sparse line
    sets (< 0.35 lines per grid point: per-level sub-linesets) by per-line expansions; 0: every evaluation exact."""
    check(lib.sr_set_far_field(int(on)), "sr_set_far_field")


_UNITS = {"Wm2": 0, "ergscm2": 1, "nWcm2": 2}


class ILS(object):
    """A tabulated instrument line shape (sr_set_ils): knots phi at the uniformly spaced reduced offsets
    t = (x - centre) / width from t_lo to t_hi, interpolated by the cubic Hermite interpolant of include/spectrobot_hip.h
    (central-difference slopes, one-sided at the ends; zero outside [t_lo, t_hi]).  phi: [n_tab], one table for all bands,
    or [n_bands, n_tab], table b for band b of the calls it is given to.  normalize: every table is divided by the exact
    integral of its interpolant over t (computed in numpy.longdouble, rounded once), so that a flat spectrum keeps its
    level whatever the band's width; a table whose area is not positive raises.  The library itself uses the knots as
    given.  Pass it as ils= to hires_to_lowres, hires_to_lowres_instrument, retrieval_forward / _step / _loop,
    limb_rays_state_bands and the state_bands methods: the call binds it, runs and unbinds."""

    def __init__(self, t_lo, t_hi, phi, normalize=True):
        phi = np.array(phi, dtype=np.float64)
        if phi.ndim not in (1, 2):
            raise ValueError("phi must be [n_tab] or [n_bands, n_tab]")
        per_band = phi.ndim == 2
        phi = np.atleast_2d(phi)
        t_lo, t_hi = float(t_lo), float(t_hi)
        if phi.shape[0] < 1 or phi.shape[1] < 4:
            raise ValueError("a line shape needs at least 4 knots per table")
        if phi.shape[1] > _lib.SR_MAX_ILS_TAB:
            raise ValueError("more than %d knots per table" % _lib.SR_MAX_ILS_TAB)
        if not (np.isfinite(t_lo) and np.isfinite(t_hi) and t_lo < t_hi):
            raise ValueError("t_lo < t_hi, both finite")
        if not np.all(np.isfinite(phi)):
            raise ValueError("a knot is not finite")
        if normalize:
            area = self.interpolant_area(t_lo, t_hi, phi)
            if not np.all(area > 0):
                raise ValueError("a table's area is not positive: nothing to normalise by")
            phi = np.asarray(phi.astype(np.longdouble) / area[:, None], np.float64)
        self.t_lo, self.t_hi, self.per_band = t_lo, t_hi, per_band
        self.phi = np.ascontiguousarray(phi)
        self.n_shapes, self.n_tab = self.phi.shape
        self.desc = _lib.IlsDesc(self.n_shapes, self.n_tab, t_lo, t_hi, self.phi.ctypes.data_as(dp))

    @staticmethod
    def interpolant_area(t_lo, t_hi, phi):
        """The exact integral of each table's interpolant in numpy.longdouble [n_shapes]:
        h (sum_k (phi_k + phi_(k+1)) / 2 + ((phi_1 - phi_0) - (phi_(n-1) - phi_(n-2))) / 12)."""
        LD = np.longdouble
        p = np.atleast_2d(np.asarray(phi, np.float64)).astype(LD)
        h = (LD(t_hi) - LD(t_lo)) / LD(p.shape[1] - 1)
        trap = p.sum(axis=1) - (p[:, 0] + p[:, -1]) / LD(2)
        return h * (trap + ((p[:, 1] - p[:, 0]) - (p[:, -1] - p[:, -2])) / LD(12))

    def area(self):
        """sr_ils_area of the table as bound: numpy [n_shapes]."""
        out = np.zeros(self.n_shapes)
        check(lib.sr_ils_area(C.byref(self.desc), out.ctypes.data_as(dp)), "sr_ils_area")
        return out

    def knots(self):
        return np.linspace(self.t_lo, self.t_hi, self.n_tab)

    def select(self, order):
        """The per-band tables in another band order (a shared table: itself)."""
        if not self.per_band:
            return self
        return ILS(self.t_lo, self.t_hi, self.phi[np.asarray(order)], normalize=False)

    @classmethod
    def from_function(cls, fn, t_lo, t_hi, n_tab, normalize=True):
        """fn(t) sampled at the n_tab knots."""
        return cls(t_lo, t_hi, fn(np.linspace(float(t_lo), float(t_hi), int(n_tab))), normalize=normalize)

    @classmethod
    def gaussian(cls, n_tab=641, t_max=5.0):
        """exp(-t^2 / 2) / sqrt(2 pi) on +-t_max, as given (not renormalised): for cross-checks against the built-in
        Gaussian with n_sigma = t_max."""
        return cls.from_function(lambda t: np.exp(-0.5 * t * t) / np.sqrt(2.0 * np.pi), -t_max, t_max, n_tab, normalize=False)

    @classmethod
    def sinc(cls, n_lobes, n_tab, apodisation=None):
        """sin(pi t) / (pi t) on +-n_lobes (the width is the distance of the first zero; the ends are zeros of the
        shape), negative side lobes and all.  apodisation: a function of u = t / n_lobes in [-1, 1] that multiplies it."""
        n_lobes = float(n_lobes)
        fn = (lambda t: np.sinc(t)) if apodisation is None else (lambda t: np.sinc(t) * apodisation(t / n_lobes))
        return cls.from_function(fn, -n_lobes, n_lobes, n_tab)


class _IlsBound(object):
    """with _IlsBound(ils): the calling thread's band calls integrate with `ils`; the Gaussian again on the way out.
    None: nothing is bound or unbound."""

    def __init__(self, ils):
        if ils is not None and not isinstance(ils, ILS):
            raise TypeError("ils must be an engine.ILS")
        self.ils = ils

    def __enter__(self):
        if self.ils is not None:
            check(lib.sr_set_ils(C.byref(self.ils.desc)), "sr_set_ils")

    def __exit__(self, *exc):
        if self.ils is not None:
            check(lib.sr_set_ils(None), "sr_set_ils")
        return False


def _lowres_call(entry, n_tab, rad, grid, centers_nm, widths_nm, out_units, n_sigma, g_lo, ils=None):
    """The instrument step's arguments, checked and marshalled once for its two entry points: returns numpy
    [n_rays, n_tab, n_bands] as `entry` (sr_hires_to_lowres_shard_dev: n_tab 1; sr_hires_to_lowres_instr_shard_dev: 3) fills it."""
    w0, step, n = grid_params(grid)
    n_sh = rad.shape[-1]
    if g_lo is None:
        if n_sh != n:
            raise ValueError("spectrum of %d points on a grid of %d (pass g_lo for the partial integrals of a shard)" % (n_sh, n))
        g_lo = 0
    assert rad.is_cuda and rad.dtype == torch.float64 and rad.is_contiguous() and 0 <= g_lo and g_lo + n_sh <= n
    rad2 = rad.reshape(-1, n_sh)
    centers_nm, cp = _d(centers_nm)
    widths_nm, wp = _d(widths_nm)
    if widths_nm.size != centers_nm.size:
        raise ValueError("{} spectral widths for {} grid points".format(widths_nm.size, centers_nm.size))
    out = np.zeros((rad2.shape[0], n_tab, centers_nm.size))
    with _IlsBound(ils):
        check(getattr(lib, entry)(C.c_void_p(rad2.data_ptr()), rad2.shape[0], n_sh, int(g_lo), w0, step, cp, wp, centers_nm.size,
                                  float(n_sigma), _UNITS[out_units], out.ctypes.data_as(dp), _stream_ptr()), entry)
    return out


def hires_to_lowres(rad, grid, centers_nm, widths_nm, out_units="Wm2", n_sigma=5.0, g_lo=None, ils=None):
    """Gaussian-ILS degradation of hi-res spectra (CUDA float64 [n_rays, n_grid], 'ergscm2' on the
    cm-1 grid) onto low-resolution bands given in nm: SpectralIntensity.hires_to_lowres
    (spect_classes.py:1180-1191).  Returns numpy [n_rays, n_bands] in out_units.
    g_lo given: rad holds the grid points g_lo .. g_lo + rad.shape[-1] - 1 only (a spectral shard) and the PARTIAL band
    integrals over them are returned (sr_hires_to_lowres_shard_dev); `grid` is always the whole grid.  Without g_lo
    the spectrum must cover the whole grid (a mis-sized spectrum is an error, not a partial integral).
    ils: an ILS, the tabulated line shape in the Gaussian's place (widths_nm scale its reduced offsets; n_sigma is not used)."""
    return _lowres_call("sr_hires_to_lowres_shard_dev", 1, rad, grid, centers_nm, widths_nm, out_units, n_sigma, g_lo, ils)[:, 0]


def hires_to_lowres_instrument(rad, grid, centers_nm, widths_nm, out_units="Wm2", n_sigma=5.0, g_lo=None, ils=None):
    """hires_to_lowres with the two instrument derivatives of every band (sr_hires_to_lowres_instr_shard_dev): returns
    (low, dlow_dcentre, dlow_dlnwidth), numpy [n_rays, n_bands] each -- the band values (hires_to_lowres's, bit for bit),
    their derivatives to a shift of the band centre (per nm) and to the logarithm of the ILS width,
        d low_b / d delta = k sum_i s_i W_i t_i / w_b,     d low_b / d eta = k sum_i s_i W_i (t_i^2 - 1),
    t_i = (x_i - f_b) / w_b, with the window's membership held fixed (it is piecewise constant in f and w; a jump is of
    relative size exp(-n_sigma^2 / 2)).  Any parametrisation of the centres and widths is a chain rule on these rows.
    Arguments as hires_to_lowres; a shard (g_lo) returns partial sums that add up over the shards.
    ils: an ILS; the two rows are then the derivatives of its interpolant, -p phi^' / w^2 and -p (phi^ + t phi^') / w."""
    out = _lowres_call("sr_hires_to_lowres_instr_shard_dev", 3, rad, grid, centers_nm, widths_nm, out_units, n_sigma, g_lo, ils)
    return out[:, 0].copy(), out[:, 1].copy(), out[:, 2].copy()


def set_table_budget(n_bytes):
    """Bytes of per-(line, layer) record tables per launch; longer layer stacks run in batches."""
    check(lib.sr_set_table_budget(int(n_bytes)), "sr_set_table_budget")
