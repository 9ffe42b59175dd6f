"""The Curtis-Godson columns of every route of the device LOS pipeline, and the VMRs a retrieval's parameter vector
gives, against the extended-precision CPU reference of tests/columns_reference.py on its case set: limb rays from
mid-shell to 1e-9 km from a level, n_sub = 1 .. 32, ragged segments, 1 to 130 segments (64 threads per block), 1 and 3
rays, 1 to 8 gases, photon and observer order.

Errors are counted in units of 2^-53 M + 1e-290, M the sum of the formula's absolute addends (the formula cancels on
the short tangent segments: a relative tolerance means nothing there).  The limit of every comparison is 8 x K_PLAIN,
K_PLAIN being what the same sums in plain numpy fp64 measure against the reference on the SAME inputs -- never what a
kernel gives.  Every test prints K_PLAIN, the limit and the worst unit count of each route before it asserts.

Group A: the routes that return columns (sr_los_columns, sr_curgod).
Group B: the columns of RESIDENT batches cannot be read through the ABI, so they are read out through the recursion.
Every segment of a ray gets a coefficient row of its own (seg_layer = arange, n_layers = n_pts = the longest ray), every
absorption coefficient is 0 and the emission coefficients of ONE gas g are the identity, emi[g][k][j] = (k == j).  Then
tau = 0 exactly, t = f = 1 (the exactly-zero optical depth the limb panel pins), and rad[r][j] = col[g][seg_off[r] + j]
with no rounding: one non-zero addend per point.  The parameter rows of the Jacobian are the parameter-mask columns in
the same way.  The read-out's own rounding is measured by limb_reference.plain_fp64 on the same tables (0) and added.
Needs a real MI355X."""
import numpy as np
import pytest

import columns_reference as C
import limb_reference as R

pytestmark = pytest.mark.gpu
LD = C.LD
GASES = {1: [2], 2: [C.ZERO_PROF, 0], 4: [0, 1, 2, 3], 5: [0, 1, 2, 3, C.ZERO_PROF], 8: [8, 7, 6, 5, C.ZERO_PROF, 3, 2, 1]}
ORDERS = ("photon", "observer")


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    from spectrobot_amd import engine
    engine.set_device(0)
    return engine


def _np(t):
    return t.detach().cpu().numpy()


class Tally(object):
    """The comparisons of one test: K_PLAIN grows with every plain() (the plain fp64 sums on the inputs of a launch),
    every route keeps its worst unit count; everything is printed before anything is asserted."""

    def __init__(self):
        self.k, self.extra, self.rows, self.fail = 0.0, 0.0, {}, []

    def plain(self, got64, ref, M):
        self.k = max(self.k, float(C.units(got64, ref, M).max()))

    def add(self, route, got, ref, M, where=""):
        u = C.units(got, ref, M)
        i = np.unravel_index(int(np.argmax(u)), u.shape) if u.size else ()
        w = float(u[i]) if u.size else 0.0
        if route not in self.rows or w > self.rows[route][0]:
            self.rows[route] = (w, "%s %s" % (where, i))

    def exact(self, what, ok):
        if not ok:
            self.fail.append(what)

    def finish(self):
        lim = C.KERNEL_MARGIN * self.k + self.extra
        print("\nK_PLAIN %.3g  limit %.3g units (read-out's own rounding: %.3g)" % (self.k, lim, self.extra))
        for route, (w, where) in self.rows.items():
            print("  %-58s %8.3g units%s at %s" % (route, w, "  OVER" if not w <= lim else "", where))
        bad = [(r, w) for r, (w, _) in self.rows.items() if not w <= lim]
        assert not bad and not self.fail, "over %.3g units: %s; not exact: %s" % (lim, bad, self.fail)


def _los(eng, b, rows, scale, order="photon"):
    return eng.LimbLOS(b["seg_off"], b["seg_layer"], b["pt_off"], b["x"], b["nd"], b["vmr"][rows], col_scale=scale, LOS_order=order)


def _reference(T, b, vmr, scale):
    """(ref, M) in long double of the batch's columns; the plain fp64 sums of the same inputs go to the tally."""
    ref, M = C.columns(2, b["x"], b["nd"], vmr, pt_off=b["pt_off"], scale=scale)
    T.plain(C.columns(2, b["x"], b["nd"], vmr, pt_off=b["pt_off"], dtype=np.float64, scale=scale)[0], ref, M)
    return ref, M


# ------------------------------------------------------------------------------------------------------------------
# Group A: direct read
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_sub", C.N_SUBS)
def test_los_columns(eng, n_sub):
    """LimbLOS.columns() (sr_los_columns: the batch staged per call) on the case set: every segment count, 1 to 8 gases
    with col_scale, both orders (observer order returns the columns in the order the batch lists its segments); last, every
    segment of the case set in one ray."""
    T = Tally()
    for counts in C.SEG_COUNTS + ((C.pool(n_sub)["x"].shape[0],),):
        b = C.batch(n_sub, counts, start=C.tangent_start(n_sub) if sum(counts) == 1 else 0)
        for n_gas, rows in GASES.items():
            scale = np.linspace(0.5, 2.0, n_gas)
            ref, M = _reference(T, b, b["vmr"][rows], scale)
            for order in ORDERS:
                got = _los(eng, b, rows, scale, order).columns()
                T.add("sr_los_columns %s, %d gases" % (order, n_gas), got, ref, M, "segments %s" % (counts,))
                T.exact("zero profile, %s %s" % (counts, order), all(np.all(got[i] == 0.0) for i, r in enumerate(rows) if r == C.ZERO_PROF))
    T.finish()


def test_los_columns_ragged(eng):
    """Segments of 2, 3, 4, 9 and 33 sample points in one pt_off (sr_los_desc takes no segment of one point: the refusal
    is checked), in one ray and in two, both orders: observer order re-packs the sample points of ragged segments."""
    T = Tally()
    pts = C.RAGGED[1:]
    for counts in ((5,), (2, 3)):
        b = C.batch(32, counts, start=C.tangent_start(32) - 1, points=pts)
        rows, scale = GASES[4], np.array([0.98827, 1.0, 0.5, 2.0])
        ref, M = _reference(T, b, b["vmr"][rows], scale)
        for order in ORDERS:
            T.add("sr_los_columns ragged %s" % order, _los(eng, b, rows, scale, order).columns(), ref, M, "rays %s" % (counts,))
    T.finish()
    b = C.batch(32, (len(C.RAGGED),), points=C.RAGGED)
    from spectrobot_amd._lib import SR_ERR_ARG, SpectRobotHipError
    with pytest.raises(SpectRobotHipError) as err:
        _los(eng, b, [0], [1.0]).columns()
    assert err.value.status == SR_ERR_ARG


def test_compat_curgods(eng):
    """compat.curgods (sr_curgod, sr_curgod_kernel) 1 .. 4: every segment of the case set in one launch per n_sub, the
    ragged batch with its one-point segment (an exact 0.0), and the f2py-shaped single calls, which read the first n_p
    values of longer arrays."""
    from spectrobot_amd.compat import curgods
    for w in (1, 2, 3, 4):
        T = Tally()
        for n_sub in C.N_SUBS:
            b = C.batch(n_sub, (C.pool(n_sub)["x"].shape[0],))
            f = b["vmr"][2]
            for row in ((0,) if w == 1 else (0, 1, 3, C.ZERO_PROF, 7)):
                v = b["vmr"][row]
                ref, M = C.columns(w, b["x"], b["nd"], v, f, b["pt_off"])
                T.plain(C.columns(w, b["x"], b["nd"], v, f, b["pt_off"], np.float64)[0], ref, M)
                got = curgods.curgod_batch(w, b["nd"], b["x"], b["pt_off"], vmr=v, f=f)
                T.add("curgod_batch %d" % w, got, ref, M, "n_sub %d profile %d" % (n_sub, row))
                if w in (2, 4) and row == C.ZERO_PROF:
                    T.exact("zero profile", np.all(got == 0.0))
        b = C.batch(32, (len(C.RAGGED),), start=C.tangent_start(32), points=C.RAGGED)
        f, v = b["vmr"][2], b["vmr"][1]
        ref, M = C.columns(w, b["x"], b["nd"], v, f, b["pt_off"])
        T.plain(C.columns(w, b["x"], b["nd"], v, f, b["pt_off"], np.float64)[0], ref, M)
        got = curgods.curgod_batch(w, b["nd"], b["x"], b["pt_off"], vmr=v, f=f)
        T.add("curgod_batch %d ragged" % w, got, ref, M)
        T.exact("one-point segment", got[0] == 0.0 and not np.signbit(got[0]))
        a, e = b["pt_off"][-2], b["pt_off"][-1]
        nd, x, v, f = b["nd"][a:e], b["x"][a:e], v[a:e], f[a:e]
        for n_p in (2, 9, 33):
            one = (curgods.curgod_fort_1(nd, x, n_p), curgods.curgod_fort_2(nd, v, x, n_p), curgods.curgod_fort_3(nd, v, f, x, n_p),
                   curgods.curgod_fort_4(nd, v, f, x, n_p))[w - 1]
            r1, M1 = C.columns(w, x[:n_p], nd[:n_p], v[:n_p], f[:n_p])
            T.plain(C.columns(w, x[:n_p], nd[:n_p], v[:n_p], f[:n_p], dtype=np.float64)[0], r1, M1)
            T.add("curgod_fort_%d" % w, np.array([one]), r1, M1, "n_p %d" % n_p)
        T.finish()


# ------------------------------------------------------------------------------------------------------------------
# Group B: read-out through the recursion
# ------------------------------------------------------------------------------------------------------------------
class ReadOut(object):
    """The one-hot coefficient tables of a batch and the unpacking of what the recursion returns."""

    def __init__(self, b, n_gas):
        import torch
        self.b, self.n_gas = b, n_gas
        self.n = int(np.diff(b["seg_off"]).max())           # n_layers = n_pts
        self.abs = torch.zeros((n_gas, self.n, self.n), dtype=torch.float64, device="cuda")
        self.emi = torch.zeros_like(self.abs)
        self.g = None

    def coeffs(self, g):
        if self.g is not None:
            self.emi[self.g].zero_()
        self.emi[g].fill_diagonal_(1.0)
        self.g = g
        return (self.abs, self.emi)

    def rows(self, a):
        """[..., n_rays, n_pts] -> ([..., n_seg] in the batch's segment order, whether all the rest is exactly 0)."""
        so = self.b["seg_off"]
        a = np.asarray(a)
        out = np.concatenate([a[..., r, :so[r + 1] - so[r]] for r in range(so.size - 1)], axis=-1)
        rest = all(np.all(a[..., r, so[r + 1] - so[r]:] == 0.0) for r in range(so.size - 1))
        return out, rest

    def rounding(self, ref, M):
        """The read-out's own rounding, in the units of the comparison: limb_reference.plain_fp64 on these tables with
        the reference's columns (rounded to fp64) of one gas."""
        so, worst = self.b["seg_off"], 0.0
        col = np.asarray(ref, np.float64)
        for r in range(so.size - 1):
            c = col[so[r]:so[r + 1]]
            S = c.size
            E = np.zeros((S, self.n))
            E[np.arange(S), np.arange(S)] = c
            z = np.zeros((0, S, self.n))
            I, _ = R.plain_fp64(np.zeros((S, self.n)), E, z, z, np.zeros(self.n))
            worst = max(worst, float(C.units(I[:S], c, np.asarray(M, LD)[so[r]:so[r + 1]]).max()), float(np.abs(I[S:]).max() if S < self.n else 0.0))
        return worst


@pytest.mark.parametrize("n_sub", C.N_SUBS)
def test_resident_batch_columns(eng, n_sub):
    """limb_rays on a resident handle (sr_los_create), photon and observer order (the re-listing), one ray of 130 segments
    and three of 1, 64 and 65; then the same handle after set_vmr (new columns) and after refresh_columns (the same
    bits)."""
    T = Tally()
    rows, new_rows, scale = GASES[4], [5, 6, 7, 8], np.array([0.98827, 1.0, 0.5, 2.0])
    for counts in ((130,), (1, 64, 65)):
        b = C.batch(n_sub, counts)
        ro = ReadOut(b, 4)
        ref, M = _reference(T, b, b["vmr"][rows], scale)
        ref2, M2 = _reference(T, b, b["vmr"][new_rows], scale)
        T.extra = max(T.extra, ro.rounding(ref[1], M[1]))
        for order in ORDERS:
            los = _los(eng, b, rows, scale, order)
            direct = los.columns()
            read = lambda: [ro.rows(_np(eng.limb_rays(ro.coeffs(g), los))) for g in range(4)]
            first = read()
            for g in range(4):
                T.add("limb_rays resident %s" % order, first[g][0], ref[g], M[g], "rays %s gas %d" % (counts, g))
                T.exact("rows beyond the ray, %s %s gas %d" % (order, counts, g), first[g][1])
                T.exact("resident == staged columns, %s %s gas %d" % (order, counts, g), np.array_equal(first[g][0], direct[g]))
            los.set_vmr(b["vmr"][new_rows])
            second = read()
            los.refresh_columns()
            third = read()
            for g in range(4):
                T.add("after set_vmr %s" % order, second[g][0], ref2[g], M2[g], "rays %s gas %d" % (counts, g))
                T.exact("refresh_columns: the same bits, %s %s gas %d" % (order, counts, g),
                        np.array_equal(second[g][0], third[g][0]) and second[g][1] and third[g][1])
            los.close()
    T.finish()


def _shuffled_par_gas(n_par, n_gas, seed):
    pg = np.arange(n_par) % n_gas
    return np.random.default_rng([20261020, seed, n_par]).permutation(pg).astype(np.int32)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("n_par", [1, 8, 9, 33])
def test_parameter_mask_columns(eng, n_par, order):
    """The rows of limb_rays_jacobian are the parameter-mask columns scale[par_gas[p]] curgod_fort_2(nd, par_w[p], x):
    through the resident batch (sr_los_create_par) and the staged call (sr_limb_rays_jac_dev), the one-pass kernels and
    the forward sensitivities (set_jac_layer_mode 1).  Parameters of three gases with different col_scales in shuffled
    order (a scale taken from the wrong gas or a row offset off by one shows), one parameter whose weights are all zero
    (exact zeros), a gas without parameters.  A launch reads out the rows of ONE gas; the rows of the other gases'
    parameters are exact zeros in it."""
    T = Tally()
    rows, scale = GASES[4], np.array([0.98827, 3.0, 0.5, 2.0])
    b = C.batch(3, (1, 64, 65))
    ro = ReadOut(b, 4)
    pg = _shuffled_par_gas(n_par, 3, 1)
    zero = [n_par // 2] if n_par > 1 else []
    W = C.hat_weights(pg, b["alt"], zero_rows=zero)
    ref, M = _reference(T, b, b["vmr"][rows], scale)
    mref, mM = C.mask_columns(b, pg, W, scale)
    T.plain(C.mask_columns(b, pg, W, scale, np.float64)[0], mref, mM)
    T.extra = ro.rounding(ref[1], M[1])
    los = _los(eng, b, rows, scale, order)
    try:
        for mode in (0, 1):
            eng.set_jac_layer_mode(mode)
            for resident in (True, False):
                tag = "%s, mode %d" % ("sr_los_create_par" if resident else "sr_limb_rays_jac_dev", mode)
                for g in range(4):
                    rad, jac = eng.limb_rays_jacobian(ro.coeffs(g), los, pg, W, resident=resident)
                    col, rest = ro.rows(_np(rad))
                    T.add("rad " + tag, col, ref[g], M[g], "gas %d" % g)
                    jr, jrest = ro.rows(np.moveaxis(_np(jac), 1, 0))       # [n_par, n_rays, n_pts] -> [n_par, n_seg]
                    mine = pg == g
                    T.add("jac " + tag, jr[mine], mref[mine], mM[mine], "gas %d" % g)
                    T.exact("zeros beyond the rays / of the other gases' parameters, %s gas %d" % (tag, g),
                            rest and jrest and np.all(jr[~mine] == 0.0))
                    T.exact("the all-zero parameter, %s gas %d" % (tag, g), np.all(jr[zero] == 0.0))
    finally:
        eng.set_jac_layer_mode(0)
        los.close()
    T.finish()


@pytest.mark.parametrize("n_par", C.N_PARS)
def test_retrieval_forward_parameter_blocks(eng, n_par):
    """retrieval_forward with band fusion off (the hi-res rows stay in `buf`): parameter vector -> VMRs
    (sr_los_vmr_from_params_kernel, the vector in blocks of 32 kernel arguments) -> columns, on columns_reference's layout:
    gas 0 has parameters in the first block only, gas 1 only beyond index 32 (its row starts in a later block), gas 2 on
    both sides of every block edge (a later block adds to the row an earlier one started), gas 3 none (its VMR is kept:
    the same bits as the staged columns).  Two parameter vectors on the same handle: the second call gives the second
    vector's columns (the rows restart, nothing is added to the first call's), the first vector again its own bits.
    rad rows against vmr_from_params + columns in long double, jac rows against the mask columns."""
    T, Tm = Tally(), Tally()
    scale = np.array(C.RETRIEVAL_SCALE)
    b = C.batch(3, (1, 64, 65))
    ro = ReadOut(b, 4)
    pg = C.retrieval_par_gas(n_par)
    W = C.hat_weights(pg, b["alt"])
    W.setflags(write=False)
    xs = [C.retrieval_x(pg, 1), C.retrieval_x(pg, 2)]
    from spectrobot_amd import synthetic as syn
    grid = syn.make_grid(2975.0, 5e-4, ro.n)
    bands, widths = np.array([1e7 / grid[ro.n // 2]]), np.array([0.02])
    refs = []
    for x in xs:
        _, _, col, M = C.chain(b, pg, W, x, scale)
        T.k = max(T.k, C.k_plain_chain(b, pg, W, x, scale)[1])
        refs.append((col, M))
    mref, mM = C.mask_columns(b, pg, W, scale)
    Tm.plain(C.mask_columns(b, pg, W, scale, np.float64)[0], mref, mM)
    T.extra = Tm.extra = ro.rounding(refs[0][0][1], refs[0][1][1])
    los = _los(eng, b, [0, 1, 2, 3], scale)
    staged = los.columns()
    n_rays = los.n_rays
    eng.set_band_fusion(False)
    try:
        buf, got = None, []
        for k in (0, 1, 0):
            per_gas = []
            for g in range(4):
                _, buf = eng.retrieval_forward(ro.coeffs(g), los, pg, W, xs[k], grid, bands, widths, buf=buf)
                a = _np(buf)
                col, rest = ro.rows(a[:n_rays])
                jr, jrest = ro.rows(np.moveaxis(a[n_rays:].reshape(n_rays, n_par, ro.n), 1, 0))
                per_gas.append((col, jr))
                call = ("first x", "second x", "first x again")[len(got)]
                T.add("rad, %s" % call, col, refs[k][0][g], refs[k][1][g], "gas %d" % g)
                mine = pg == g
                if mine.any():
                    Tm.add("jac, %s" % call, jr[mine], mref[mine], mM[mine], "gas %d" % g)
                T.exact("zeros, %s gas %d" % (call, g), rest and jrest and np.all(jr[~mine] == 0.0))
            got.append(per_gas)
        for g in range(4):
            T.exact("the first x again: its own bits, gas %d" % g,
                    np.array_equal(got[0][g][0], got[2][g][0]) and np.array_equal(got[0][g][1], got[2][g][1]))
        for k in range(3):
            T.exact("gas 3 keeps its VMR bit for bit (call %d)" % k, np.array_equal(got[k][3][0], staged[3]))
        for g in range(3):
            if np.any(pg == g):
                T.exact("gas %d: the second x changes the columns" % g, not np.array_equal(got[0][g][0], got[1][g][0]))
            else:
                T.exact("gas %d has no parameters: the staged columns" % g, np.array_equal(got[0][g][0], staged[g]))
    finally:
        eng.set_band_fusion(True)
        los.close()
    print("\nrad rows (units of the chain: the columns' M + what 2^-53 sum |x_p w_p| of the VMRs does to a column):")
    try:
        T.finish()
    finally:
        print("jac rows (the mask columns):")
        Tm.finish()


def test_eight_gas_batch_hands_the_same_columns_on(eng):
    """Eight gases (sr_limb_many.hip's host path): limb_rays on the resident batch and limb_rays_state_jacobian with
    column parameters of four of the gases."""
    T = Tally()
    rows, scale = GASES[8], np.linspace(0.5, 2.0, 8)
    b = C.batch(3, (1, 64, 65))
    ro = ReadOut(b, 8)
    pg = np.array([7, 0, 4, 3, 7, 0, 5, 3, 5], np.int32)
    W = C.hat_weights(pg, b["alt"], zero_rows=[4])
    ref, M = _reference(T, b, b["vmr"][rows], scale)
    mref, mM = C.mask_columns(b, pg, W, scale)
    T.plain(C.mask_columns(b, pg, W, scale, np.float64)[0], mref, mM)
    T.extra = ro.rounding(ref[0], M[0])
    for order in ORDERS:
        los = _los(eng, b, rows, scale, order)
        for g in range(8):
            col, rest = ro.rows(_np(eng.limb_rays(ro.coeffs(g), los)))
            T.add("limb_rays, 8 gases, %s" % order, col, ref[g], M[g], "gas %d" % g)
            T.exact("rows beyond the ray, %s gas %d" % (order, g), rest)
            rad, jac = eng.limb_rays_state_jacobian(ro.coeffs(g), los, par_gas=pg, par_w=W)
            col, rest = ro.rows(_np(rad))
            T.add("state rad, 8 gases, %s" % order, col, ref[g], M[g], "gas %d" % g)
            jr, jrest = ro.rows(np.moveaxis(_np(jac), 1, 0))
            mine = pg == g
            if mine.any():
                T.add("state jac, 8 gases, %s" % order, jr[mine], mref[mine], mM[mine], "gas %d" % g)
            T.exact("zeros, state %s gas %d" % (order, g), rest and jrest and np.all(jr[~mine] == 0.0) and np.all(jr[4] == 0.0))
        los.close()
    T.finish()
