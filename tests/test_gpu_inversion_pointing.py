"""retrieval.inversion_state with the pointing in the state (retrieval.Pointing, the set named "pointing": one tangent-
altitude offset common to all pixels, beside a VMR profile) on its two routes -- the one fused call with the pointing row
(bands_in_kernel=True) and the state Jacobian call plus the instrument step -- on a noise-free twin, and one iteration's
pointing column against central differences of the driver's own forward model.  The scene is the small mixed scene of
tests/test_gpu_state_bands.py (6000 points, 22 layers, an LTE HCN and a non-LTE CH4, five pixels with the closed-form
field of view).  Needs a real MI355X."""
import copy

import numpy as np
import pytest

import limb_reference as R
import pointing_reference as P

pytestmark = pytest.mark.gpu
SIGMA_KM = 4.0                    # the a-priori error of the offset
TRUE_OFFSET = 0.5 * SIGMA_KM
H_KM = 1e-3                       # the step of the central differences


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    from spectrobot_amd import engine
    engine.set_device(0)
    return engine


def _sets(scene, offset=None, profile=None, pointing_first=False):
    from spectrobot_amd import retrieval, spect_main_module as smm
    z = scene.z
    span = z[-1] - z[0]
    nodes = [z[0] + q * span for q in (0.1, 0.45, 0.8)]
    apr, sig = np.full(3, 2.2e-6), np.full(3, 1.1e-6)
    bs = smm.BayesSet(tag="HCN + pointing offset")
    sets = [smm.LinearProfile_1D_new("HCN", z, nodes, apr, sig, first_guess_prof=profile),
            retrieval.Pointing((0.0, SIGMA_KM) if offset is None else (0.0, SIGMA_KM, offset))]
    for st in (sets[::-1] if pointing_first else sets):
        bs.add_set(st)
    return bs, np.concatenate([sig, [SIGMA_KM]])


def _twin(eng):
    """Observations (noise-free) from a perturbed truth: the HCN profile scaled by 1.3, every line of sight TRUE_OFFSET km
    higher than the pixels say.  Returns scene, pixels, x_true in the order (profile, offset)."""
    import test_gpu_state_bands as SB
    from spectrobot_amd import retrieval
    scene, pixels = SB._mixed_scene(eng)
    x_true = np.concatenate([1.3 * np.full(3, 2.2e-6), [TRUE_OFFSET]])
    truth, _ = _sets(scene, profile=x_true[:3])
    retrieval._state_into_gases(scene, truth)
    moved = [retrieval.LimbPixel(p.limb_tg_alt + TRUE_OFFSET, fov_half=p.fov_half, pixel_rot=p.pixel_rot) for p in pixels]
    SB._observe(scene, moved, 0.004)
    for p, m in zip(pixels, moved):
        p.observation, p.noise = m.observation, m.noise
    return scene, pixels, x_true


@pytest.mark.parametrize("fused", [True, False])
def test_noise_free_twin(eng, fused):
    """From the a priori (offset 0): chi square falls, the offset and the profile end nearer the truth than they began,
    the loop converges, and the retrieved offset lies within its own posterior sigma (the stored covariance) of the truth."""
    from spectrobot_amd import retrieval
    scene, pixels, x_true = _twin(eng)
    bs, sigma = _sets(scene)
    before = np.abs(bs.param_vector() - x_true) / sigma
    chi, _, sims, b = retrieval.inversion_state(scene, copy.deepcopy(bs), pixels, max_it=12, bands_in_kernel=fused)
    after = np.abs(b.param_vector() - x_true) / sigma
    post = float(np.sqrt(b.VCM[3, 3]))
    print("\npointing twin (bands in kernel %d): %d iterations (%s), chi square %s; retrieved %s, truth %s; offset error %.3g km, "
          "posterior sigma %.3g km" % (fused, len(b.history), b.stop, np.array2string(np.array(b.history), precision=4),
                                       np.array2string(b.param_vector(), precision=4), np.array2string(x_true, precision=4),
                                       abs(b.param_vector()[3] - x_true[3]), post))
    assert len(b.history) >= 2 and b.history[-1] < b.history[0]
    assert after[3] < before[3] and np.linalg.norm(after[:3]) < np.linalg.norm(before[:3])
    assert b.stop == 'converged'
    assert abs(b.param_vector()[3] - x_true[3]) <= post
    assert len(sims) == len(pixels) and b.jacobian.shape == (len(pixels) * len(scene.bands_nm), 4)
    assert b.sets["pointing"].offset() == b.param_vector()[3]


def _chain_truncation(eng, scene, pixels, h):
    """The analytic-against-difference distance of the long double chain on this scene at step h: the helper's geometry
    and columns and limb_reference.recursion_reference on the scene's coefficient tables (fp64 data), the rows brought to
    the bands and through the field of view by the fp64 instrument step (its rounding, 1e-15, is far below the truncation
    that is measured).  max |analytic - difference| / max |analytic| over pixels and bands."""
    import torch
    from spectrobot_amd import spect_main_module as smm
    a, e = (t.cpu().numpy() for t in scene.coefficient_stack())
    vmr = np.array([g.vmr for g in scene.gases])
    scale = np.array([g.iso_ratio for g in scene.gases]).astype(P.LD)[:, None]
    zero = np.zeros(a.shape[2])
    rows, diffs = [], []
    for zt in [q for p in pixels for q in p.los_alts()]:
        shells = P.crossed_shells(scene.z, zt, scene.R)
        G = P.geometry_ld(scene.z, scene.nd, vmr, zt, R=scene.R, n_sub=scene.n_sub, shells=shells)

        def forms(g, du):
            u = P.columns(g["x"], g["nd"], g["vmr"]) * scale
            tau, E = R.products(a[:, G["k"]], u, R.LD), R.products(e[:, G["k"]], u, R.LD)
            if du is None:
                none = np.zeros((0,) + tau.shape, R.LD)
                return tau, E, none, none
            dtau = np.array([a[q, G["k"]].astype(R.LD) * du[q][:, None] for q in range(len(du))])
            dE = np.array([e[q, G["k"]].astype(R.LD) * du[q][:, None] for q in range(len(du))])
            return tau, E, dtau, dE

        rad = lambda at: R.recursion_reference(*forms(P.geometry_ld(scene.z, scene.nd, vmr, at, R=scene.R, n_sub=scene.n_sub,
                                                                    shells=shells), None), zero, want_cond=False)["I"]
        diffs.append(np.asarray((rad(P.LD(zt) + P.LD(h)) - rad(P.LD(zt) - P.LD(h))) / P.LD(2 * h), np.float64))
        rows.append(np.asarray(R.recursion_reference(*forms(G, P.dcol_reference(G) * scale), zero, want_cond=False)["J"].sum(axis=0),
                               np.float64))
    rots = [p.pixel_rot for p in pixels]
    low = lambda v: eng.hires_to_lowres(torch.tensor(np.array(v), device="cuda"), scene.grid, scene.bands_nm, scene.widths_nm,
                                        out_units=scene.out_units)
    k, d = (smm.fov_closed_form(v[0::3], v[1::3], v[2::3], rots) for v in (low(rows), low(diffs)))
    return float(np.abs(k - d).max() / np.abs(k).max())


def test_pointing_column_against_central_differences(eng):
    """One iteration at the first guess on both routes: the two routes' Jacobians agree, the pointing column stands where
    the set stands (first or last in the BayesSet), and it agrees with (F(offset + h) - F(offset - h)) / 2h of the
    driver's own forward model, h = 1e-3 km, within 10 x the same distance of the long double chain on this scene plus
    2^-50 max |F| / h, relative to the column's largest element.

    Measured 2026-10-19 on an MI355X: long double chain 3.28e-10, limit 3.36e-09, composed route 3.35e-10, fused route
    3.35e-10; the two routes' columns agree to 3.5e-16 of a column's largest element."""
    from spectrobot_amd import retrieval
    scene, pixels, _ = _twin(eng)
    n_obs = len(pixels) * len(scene.bands_nm)
    out = {}
    for fused in (False, True):
        for first in (False, True):
            bs, _ = _sets(scene, pointing_first=first)
            chi, _, sims, b = retrieval.inversion_state(scene, bs, pixels, max_it=1, bands_in_kernel=fused)
            assert b.jacobian.shape == (n_obs, 4) and [p.nameset for p in b.params()][0 if first else 3] == "pointing"
            K = b.jacobian.copy()
            out[fused, first] = K[:, [1, 2, 3, 0]] if first else K
        assert np.array_equal(out[fused, True], out[fused, False])        # (the column moves with its set, nothing else changes)
    K_u, K_f = out[False, False], out[True, False]
    col_max = np.abs(K_u).max(axis=0)
    dist = np.abs(K_f - K_u).max(axis=0) / col_max
    print("\npointing set, one iteration: |K fused - K composed| per column / the column's largest element: %s" % np.array2string(dist, precision=2))
    assert np.all(col_max > 0) and np.all(dist <= 1e-11)

    def forward(offset):
        bs, _ = _sets(scene, offset=offset)
        _, _, sims, _ = retrieval.inversion_state(scene, bs, pixels, max_it=1, bands_in_kernel=False)
        return np.concatenate([s.spectrum for s in sims])

    up, down = forward(H_KM), forward(-H_KM)
    fd = (up - down) / (2.0 * H_KM)
    retrieval._state_into_gases(scene, _sets(scene)[0])                    # the first guess's profiles, for the chain
    chain = _chain_truncation(eng, scene, pixels, H_KM)
    limit = 10.0 * chain + 2.0 ** -50 * float(np.abs(up).max()) / H_KM / float(np.abs(K_u[:, 3]).max())
    bad = []
    for tag, K in (("composed", K_u), ("fused", K_f)):
        err = float(np.abs(K[:, 3] - fd).max() / np.abs(K[:, 3]).max())
        print("  %-9s |K - central difference| / largest element = %.3g (long double chain %.3g, limit %.3g)" % (tag, err, chain, limit))
        if not err <= limit:
            bad.append((tag, err, limit))
    assert not bad, bad
