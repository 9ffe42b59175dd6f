"""Host side of the vibrational-temperature Jacobian (no GPU): the closed-form d pop_L / d Tvib_L, the triangular
weights of a level's profile on the coefficient rows, and the ABI surface of sr_limb_rays_jac_level_dev."""
import ctypes as C

import numpy as np
import pytest

from spectrobot_amd import _lib
from spectrobot_amd import spect_classes as sc

E_LEV = np.array([0., 1311., 1533., 2587., 2612., 2830., 2846., 2917., 3019., 3062., 3065., 4223.])


def _case(n_steps=9, seed=2):
    rng = np.random.default_rng(seed)
    T = rng.uniform(130.0, 180.0, n_steps)
    tv = T[None, :] + rng.uniform(0.0, 45.0, (E_LEV.size, n_steps))
    q = rng.uniform(400.0, 700.0, n_steps)
    return T, tv, q


def test_dtvib_is_the_derivative_of_the_population():
    """Against the central difference in tvib of exp(-c2 E / tvib) / q, h = 1e-3 K, relative 1e-6 (as the LTE check of
    test_combine_temperature_derivative); exactly zero for the level of energy 0."""
    _, tv, q = _case()
    d = sc.level_populations_dtvib(E_LEV, tv, q)
    assert d.shape == (tv.shape[1], E_LEV.size)
    h = 1e-3
    pop = lambda t: (np.exp(-sc.c2 * E_LEV[:, None] / t) / q[None, :]).T
    fd = (pop(tv + h) - pop(tv - h)) / (2 * h)
    assert np.all(d[:, 0] == 0.0)
    assert np.max(np.abs(d[:, 1:] - fd[:, 1:]) / np.abs(fd[:, 1:])) < 1e-6
    # the closed form itself
    assert np.allclose(d, pop(tv) * (sc.c2 * E_LEV[None, :] / tv.T ** 2), rtol=1e-14, atol=0.0)


def test_dtvib_refuses_lte_and_an_iso_molecule_without_levels():
    _, tv, q = _case()
    with pytest.raises(ValueError):
        sc.level_populations_dtvib(E_LEV, None, q)
    with pytest.raises(ValueError):
        sc.level_populations_dtvib([], tv, q)
    with pytest.raises(ValueError):
        sc.level_populations_dtvib(E_LEV, tv[:5], q)


def test_lineset_method_delegates_with_the_partition_sum_of_level_populations():
    """LineSet.level_populations_dtvib supplies Q as level_populations does (no device needed: neither touches the
    handle), so d pop / d Tvib = pop c2 E / Tvib^2 of the method's own populations, with and without q_part."""
    from spectrobot_amd import engine

    class _LS(object):     # the two methods use mol / iso / level_energies only
        mol, iso, level_energies = 6, 1, E_LEV
        level_populations = engine.LineSet.level_populations
        level_populations_dtvib = engine.LineSet.level_populations_dtvib

    T, tv, q = _case()
    ls = _LS()
    for qp in (None, q):
        pop = ls.level_populations(T, tvib=tv, q_part=qp)
        d = ls.level_populations_dtvib(T, tv, q_part=qp)
        assert np.allclose(d, pop * (sc.c2 * E_LEV[None, :] / tv.T ** 2), rtol=1e-13, atol=0.0)
    with pytest.raises(ValueError):
        ls.level_populations_dtvib(T, None)
    ls.level_energies = np.zeros(0)
    with pytest.raises(ValueError):
        ls.level_populations_dtvib(T, tv)


def test_level_node_weights_are_a_partition_of_unity_inside_the_nodes():
    from spectrobot_amd import engine
    nodes = [150.0, 260.0, 400.0, 520.0, 700.0]
    alt = np.concatenate([np.linspace(100.0, 890.0, 57), [150.0, 400.0, 700.0, 330.0]])     # unsorted, nodes included
    W = engine.level_node_weights(nodes, alt)
    assert W.shape == (5, alt.size)
    inside = (alt >= nodes[0]) & (alt <= nodes[-1])
    assert inside.sum() > 30
    assert np.max(np.abs(W[:, inside].sum(axis=0) - 1.0)) < 1e-14
    assert np.all(W >= 0.0) and np.all(W <= 1.0)
    assert np.all((W[:, inside] > 0).sum(axis=0) <= 2)          # at most two nodes per row
    # a profile linear between the nodes is reproduced
    vals = np.array([3.0, -1.0, 4.0, 1.0, 5.0])
    assert np.max(np.abs(vals @ W[:, inside] - np.interp(alt[inside], nodes, vals))) < 1e-12
    # continued with the end values outside
    assert np.all(W[0, alt < nodes[0]] == 1.0) and np.all(W[-1, alt > nodes[-1]] == 1.0)
    with pytest.raises(ValueError):
        engine.level_node_weights([300.0], alt)


def test_abi_surface_of_the_level_jacobian():
    res, args = _lib.SYMBOLS["sr_limb_rays_jac_level_dev"]
    assert res is C.c_int and len(args) == 16
    assert args[4] == C.POINTER(_lib.LosDesc) and args[3] is C.c_int64
    assert hasattr(_lib.lib, "sr_limb_rays_jac_level_dev")
    assert _lib.lib.sr_abi_version() == 1
