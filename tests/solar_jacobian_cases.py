"""The low-sun scene of the solar-attenuation Jacobian tests (tests/test_gpu_solar_jacobian_scene.py): the CH4 + sunlit
haze scene of solar_source_cases with the sun near the horizon, so that the solar optical depth reaches order 1 in the line
cores and the derivative of the radiances through it is a visible part of the VMR Jacobian.  A helper module: no fixture,
no pytest setting."""
import numpy as np

import absorber_table_cases as K
import solar_source_cases as SC

SZA_DEG, PHASE_DEG = 80.0, 60.0


def low_sun_scene(eng, sza_deg=SZA_DEG):
    """SC.solar_scene with the sun at sza_deg."""
    from spectrobot_amd import retrieval, geometry
    base = K.haze_scene(eng)
    ch4, haze0 = base.gases
    haze = retrieval.TableGas("haze", haze0.table, SC.HAZE_SCALE * haze0.vmr, solar=dict(albedo=SC.ALBEDO, g=SC.ASYMMETRY))
    sun = retrieval.Sun(sza_deg, PHASE_DEG, geometry.solar_irradiance(base.grid))
    return retrieval.LimbScene(base.grid, base.z, base.temps, base.press, [ch4, haze], base.bands_nm, base.widths_nm, sun=sun)


def low_sun_twin(eng, sza_deg=SZA_DEG):
    """SC.solar_twin on the low-sun scene: (scene, pixels, bayes, x_true, sigma), the same nodes, a priori and truth."""
    from spectrobot_amd import retrieval, spect_main_module as smm
    scene = low_sun_scene(eng, sza_deg)
    z = scene.z
    span = z[-1] - z[0]
    ch4_nodes, haze_nodes, _ = K.nodes(z)
    apr = {"CH4": np.full(3, 1.3e-4), "haze": SC.HAZE_SCALE * np.array([0.7, 0.45, 0.2])}
    sig = {"CH4": 0.5 * apr["CH4"], "haze": 0.5 * apr["haze"]}
    truth = {"CH4": np.array([1.7e-4, 1.5e-4, 1.15e-4]), "haze": SC.HAZE_SCALE * np.array([1.0, 0.55, 0.14])}
    nd = {"CH4": ch4_nodes, "haze": haze_nodes}
    pixels = [retrieval.LimbPixel(z[0] + (0.03 + 0.09 * i) * span, fov_half=0.01 * span, pixel_rot=10.0 * (i % 3)) for i in range(6)]

    def bayes(values=apr):
        bs = smm.BayesSet(tag="CH4 + sunlit haze, low sun")
        for name in ("CH4", "haze"):
            bs.add_set(smm.LinearProfile_1D_new(name, z, nd[name], apr[name], sig[name], first_guess_prof=values[name]))
        return bs

    retrieval._state_into_gases(scene, bayes(truth))
    for pix, y in zip(pixels, retrieval.radtrans(scene, pixels)):
        s = 0.004 * np.abs(y.spectrum).max() * np.ones_like(y.spectrum)
        pix.observation, pix.noise = retrieval.Spectrum(y.spectrum.copy(), scene.bands_nm), retrieval.Spectrum(s, scene.bands_nm)
    return (scene, pixels, bayes, np.concatenate([truth["CH4"], truth["haze"]]), np.concatenate([sig["CH4"], sig["haze"]]))
