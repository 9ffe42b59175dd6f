#!/usr/bin/env python3
"""The solar attenuation in the Jacobians: a CH4 + sunlit haze limb scene with the sun low, retrieved twice
by retrieval.inversion_state from the same noise-free pixels -- with the Jacobians holding the solar attenuation fixed
within an iteration (the default), and with solar_attenuation=True, which adds the derivative of the radiances through the
solar optical depth to the VMR columns of every iteration's Jacobian.  Prints both chi square histories and the first
Jacobians' largest difference per column.  The scene is the synthetic one of the tests (tests/solar_jacobian_cases.py).
Needs an MI355X:  python examples/retrieve_solar_attenuation.py"""
import copy
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import solar_jacobian_cases as JC
    from spectrobot_amd import engine, retrieval
    engine.set_device(0)
    first = {}
    for flag in (False, True):
        scene, pixels, bayes, x_true, sigma = JC.low_sun_twin(engine)
        _, _, _, one = retrieval.inversion_state(scene, copy.deepcopy(bayes()), pixels, max_it=1, solar_attenuation=flag)
        first[flag] = np.array(one.jacobian)
        _, _, _, b = retrieval.inversion_state(scene, bayes(), pixels, max_it=10, lambda_LM=0.0, solar_attenuation=flag)
        d = np.abs(b.param_vector() - x_true) / sigma
        print("solar_attenuation=%s: %d iterations (%s), chi square %s\n  distance to the truth in a-priori sigmas %s"
              % (flag, len(b.history), b.stop, np.array2string(np.array(b.history), precision=4), np.array2string(d, precision=4)))
    rel = np.abs(first[True] - first[False]).max(axis=0) / np.abs(first[True]).max(axis=0)
    print("first Jacobian, the term's share of every column (largest element, relative to the column's largest): %s"
          % np.array2string(rel, precision=3))


if __name__ == "__main__":
    main()
