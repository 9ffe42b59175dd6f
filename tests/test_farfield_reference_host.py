"""The far field's truncation bound held against an extended-precision model of one line's expansion over one box
(tests/farfield_reference.py), on the host: the series reproduces the rational, the closed forms of a 1/x^2 wing match
it, and THE CONTRACT -- at the nearest distance the library admits (sr_far_field_min_distance, the kernels' own
expression), over levels 0-4 x seven (xstep, ry) x three positions of the line's centre inside its grid cell, the
truncated series is within sr_far_field_truncation_bound() = 18 x 4^-20 = 1.637e-11 of the line's own value at every
point of the box.  No GPU.

Worst case per level (all at xstep 2, ry 1e-3, the centre half a point towards the box, the outermost point AWAY from
the line), measured 2026-10-18 at degree 19:

    level   at 4 h + pm (the rule before the margin)   at sr_far_field_min_distance
      0                 1.362e-11                             1.362e-11   (unchanged: no margin at level 0)
      1                 1.795e-11                             1.217e-11
      2                 2.060e-11                             1.423e-11
      3                 2.207e-11                             1.523e-11
      4                 2.284e-11                             1.577e-11

The middle column is what the contract test reported before levels >= 1 got their margin of 0.0735 half-widths
(sr_kernels.hpp, ff_thr2): over the bound from level 1 upwards, as the closed form (d + 2 + (d + 1) r) r^(d+1) =
26 x 4^-20 = 2.36e-11 at r = 1/4 says it must be.  test_contract_needs_the_margin keeps that column alive.
"""
import numpy as np
import pytest

import farfield_reference as F


@pytest.fixture(scope="module")
def engine():
    from spectrobot_amd import engine
    return engine


@pytest.fixture(scope="module")
def degree(engine):
    return engine.far_field_degree()


def _panel():
    for level in F.LEVELS:
        for xstep, ry in F.PANEL:
            for off in F.OFFSETS:
                yield level, xstep, ry, off


def test_min_distance_entry_point(engine):
    """sr_far_field_min_distance: declared, bound, a multiple of 1/2, level 0 exactly 4 half-widths + the pole margin,
    wider levels at least that, monotone in both arguments, out-of-range arguments refused."""
    from spectrobot_amd import _lib
    assert "sr_far_field_min_distance" in _lib.SYMBOLS and _lib.lib.sr_abi_version() == 1
    for pm in (0, 2, 285):
        assert engine.far_field_min_distance(0, pm) == 128.0 + pm
        prev = 0.0
        for level in F.LEVELS:
            d = engine.far_field_min_distance(level, pm)
            assert d * 2 == int(d * 2) and d >= 4 * (32 << level) + pm and d > prev
            assert engine.far_field_min_distance(level, pm + 1) == d + 1
            # ownership must stay monotone down the hierarchy: a parent's admissible distance, less the half-width of
            # the child (the two centres' distance), is admissible for the child
            if level > 0:
                assert d - (32 << (level - 1)) >= prev
            prev = d
    assert _lib.lib.sr_far_field_min_distance(5, 2) == -1.0 and _lib.lib.sr_far_field_min_distance(-1, 2) == -1.0
    assert _lib.lib.sr_far_field_min_distance(0, -1) == -1.0
    with pytest.raises(ValueError):
        engine.far_field_min_distance(7, 2)


def test_series_reproduces_the_rational_at_degree_60():
    """At degree 60 the truncation is (1/4)^61 ~ 1e-37: what is left is the long-double rounding of the recurrence and
    of Horner's rule (measured: 8 units of 2^-63; allowed: 1000)."""
    worst = 0.0
    for level, xstep, ry, off in _panel():
        d = 4 * (32 << level) + F.pole_margin(xstep)
        worst = max(worst, F.truncation(level, xstep, ry, d, 60, off))
    print("series at degree 60 against the rational: %.3g (long double eps %.3g)" % (worst, np.finfo(F.LD).eps))
    assert worst <= 1000 * float(np.finfo(F.LD).eps)


@pytest.mark.parametrize("degree_", [19, 22])
def test_closed_forms_match_the_series_on_an_inverse_square_wing(degree_):
    """ry = 100 on a grid 2000 dw' coarse: (ry / x)^2 <= 2.7e-7 over the box (the remainder feels it about 80 times as
    much), the wing is 1/x^2, and the series' error at the two ends t = -1 / +1 of the box is the closed form to 1e-3."""
    for level in F.LEVELS:
        for r in (0.25, 0.2455, 0.2):
            h = 32 << level
            s, w, _ = F.box_series(level, 2000.0, 100.0, h / r, degree_, t=[-1.0, 1.0])
            got = np.abs(s - w) / np.abs(w)
            want = F.remainder_inverse_square(r, degree_)
            assert abs(float(got[0]) / want[0] - 1) < 1e-3 and abs(float(got[1]) / want[1] - 1) < 1e-3, (level, r, got, want)
    near, far = F.remainder_inverse_square(0.25, 19)
    assert abs(near / 4.0 ** -20 - 16) < 1e-12 and abs(far / 4.0 ** -20 - 26) < 1e-12


def _worst_per_level(degree_, distance_of):
    out = {}
    for level, xstep, ry, off in _panel():
        err, t = F.truncation(level, xstep, ry, distance_of(level, xstep), degree_, off, where=True)
        if err > out.get(level, (0.0,))[0]:
            out[level] = (err, xstep, ry, off, t)
    return out


def test_contract_truncation_at_the_admissible_distance_is_within_the_bound(engine, degree):
    """THE CONTRACT (module docstring).  The distance comes from the library, the bound comes from the library."""
    bound = engine.far_field_truncation_bound()
    worst = _worst_per_level(degree, F.min_distance)
    for level in F.LEVELS:
        print("level %d: %.4g of bound %.4g at xstep %g ry %g offset %+g t %+.5f" % ((level, worst[level][0], bound) + worst[level][1:]))
    for level in F.LEVELS:
        assert worst[level][0] <= bound, (level, worst[level], bound)


def test_contract_needs_the_margin(engine, degree):
    """The same panel at 4 half-widths + pole margin, no more: level 0 holds (there that IS the library's distance),
    every wider level misses the bound -- the margin of levels >= 1 is not slack."""
    bound = engine.far_field_truncation_bound()
    worst = _worst_per_level(degree, lambda level, xstep: 4 * (32 << level) + F.pole_margin(xstep))
    for level in F.LEVELS:
        print("level %d at 4 h + pm: %.4g of bound %.4g" % (level, worst[level][0], bound))
    assert worst[0][0] <= bound and F.min_distance(0, 2.0) == 128 + F.pole_margin(2.0)
    for level in F.LEVELS[1:]:
        assert worst[level][0] > bound, (level, worst[level])
        # and the library's margin is the closed form's, not more than a point beyond it: (4 + 0.0736) half-widths
        if degree == 19:
            assert 0.0 <= F.min_distance(level, 2.0) - (4.0735 * (32 << level) + F.pole_margin(2.0)) <= 1.0


def test_k_plain_far_recorded_and_respected(engine, degree):
    live, at = 0.0, None
    for level, xstep, ry, off in _panel():
        u = F.plain_rounding(level, xstep, ry, F.min_distance(level, xstep), degree, off)
        if u > live:
            live, at = u, (level, xstep, ry, off)
    print("K_PLAIN_FAR live: %.3g units of 2^-53 at level %d xstep %g ry %g offset %+g" % ((live,) + at))
    assert live <= F.K_PLAIN_FAR
    # the constant is a record, not a budget
    assert F.K_PLAIN_FAR <= 2.0 * F.K_PLAIN_FAR_MEASURED
    # and rounding is small change beside the bound it is added to: 8 x K x 2^-53 < 1 % of 1.6e-11
    if degree == 19:
        assert F.KERNEL_MARGIN * F.K_PLAIN_FAR * F.EPS53 < 0.01 * engine.far_field_truncation_bound()
