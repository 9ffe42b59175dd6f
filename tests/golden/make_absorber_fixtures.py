"""Writes the synthetic fixtures of the table readers (spect_classes.read_xsc / read_cia) next to this file:
absorber_sample.xsc, absorber_sample.cia, absorber_irregular.cia.  They follow HITRAN's fixed-width layouts as its
documentation gives them; the numbers are formulas, not data of any molecule.  `python make_absorber_fixtures.py` rewrites
the files; the tests import xsc_sets() / cia_sets() for what the readers must return."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# (T / K, P / Torr, nu_min, nu_max, points)
XSC = [(180.0, 20.0, 2900.0, 2903.0, 25), (220.0, 20.0, 2900.0, 2903.0, 25), (180.0, 100.0, 2900.5, 2902.5, 17),
       (250.0, 100.0, 2900.0, 2903.0, 31)]
# (T / K, nu_min, step, points)
CIA = [(80.0, 2890.0, 0.5, 41), (120.0, 2890.0, 0.5, 41), (160.0, 2895.0, 1.0, 16)]


def _xsc_values(k, n):
    i = np.arange(n)
    v = 1e-20 * (1.0 + 0.1 * k) * np.exp(-0.5 * ((i - 0.4 * n) / (0.2 * n)) ** 2) + 3e-23 * (i % 3)
    return np.array([float("%10.3E" % x) for x in v])


def _cia_values(k, n):
    i = np.arange(n)
    v = 2e-46 * (1.0 + 0.3 * k) * (1.0 + np.cos(0.3 * i)) - 3e-48   # (negative near i = 10, 31: real files carry small negatives)
    return np.array([float("%10.3E" % x) for x in v])


def xsc_sets():
    """[(T, v0, dv, values, P / hPa)] as read_xsc must return them."""
    return [(t, lo, (hi - lo) / (n - 1), _xsc_values(k, n), p * 1.333224) for k, (t, p, lo, hi, n) in enumerate(XSC)]


def cia_sets():
    return [(t, lo, dv, _cia_values(k, n)) for k, (t, lo, dv, n) in enumerate(CIA)]


def write():
    with open(os.path.join(HERE, "absorber_sample.xsc"), "w") as f:
        for k, (t, p, lo, hi, n) in enumerate(XSC):
            v = _xsc_values(k, n)
            f.write("%20s%10.4f%10.4f%7d%7.1f%6.1f%10.3E%5.3f%15s%4s%3s%3d\n" % ("SYNTH", lo, hi, n, t, p, v.max(), 0.015, "synthetic", "", "N2", 0))
            for a in range(0, n, 10):
                f.write("".join("%10.3E" % x for x in v[a:a + 10]) + "\n")
    for name, irregular in (("absorber_sample.cia", False), ("absorber_irregular.cia", True)):
        with open(os.path.join(HERE, name), "w") as f:
            for k, (t, lo, dv, n) in enumerate(CIA):
                v = _cia_values(k, n)
                nu = lo + dv * np.arange(n)
                if irregular and k == 1:
                    nu[7] += 0.01 * dv
                f.write("%20s%10.3f%10.3f%7d%7.1f%10.3E%6.3f%27s%3d\n" % ("N2-SYNTH", nu[0], nu[-1], n, t, v.max(), -0.999, "synthetic", 0))
                for x, y in zip(nu, v):
                    f.write("%10.4f %10.3E\n" % (x, y))


if __name__ == "__main__":
    write()
