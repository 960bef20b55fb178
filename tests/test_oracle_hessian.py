"""The oracle's side of the entrywise Hessian rule (tests/_hessian_cases.py), on the CPU alone:

  * orpm_eval_h still computes what it computed before orpm_eval_h_mag shared its walk (recorded bits);
  * orpm_eval_h_mag bounds |H| entrywise, is even in lambda and sigma, and is 0 only where H is 0;
  * C_NOISE covers 8 x the noise between two builds of the oracle (-ffp-contract=off against -mfma -ffp-contract=fast),
    measured over every case, step, iterate and draw the device tests use — and profiles/hessian_noise.json says the same;
  * at step 1e-3 the rule pins at least 70 % of every case's nonzero reference entries to 1e-6 of their own value.
"""
import importlib.util
import json
import os

import numpy as np
import pytest

import _hessian_cases as hc
from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
ALL = hc.CASES + hc.ANALYTIC_CASES
ALL_IDS = [c[0] for c in ALL]


def _golden_module():
    spec = importlib.util.spec_from_file_location("make_hessian_golden", os.path.join(HERE, "golden", "make_hessian_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize("name", sorted(_golden_module().CASES))
def test_eval_h_is_bit_identical_to_the_recording(built, name):
    mh = _golden_module()
    z = np.load(os.path.join(HERE, "golden", "hessian", "eval_h.npz"))
    for step, an in mh.VARIANTS:
        o = orc.Oracle(mh.CASES[name](), mh.options(step, an))
        x, lam = mh.inputs(o)
        for sigma in (0.7, 0.0):
            assert np.array_equal(o.eval_h(x, sigma, lam), z[mh.key(name, step, an, sigma)]), (step, an, sigma)


@pytest.mark.parametrize("cid,name,make", ALL, ids=ALL_IDS)
def test_mag_bounds_the_hessian_and_is_even(built, cid, name, make):
    for step in hc.STEPS:
        o = orc.Oracle(make(), hc.exact_options(step, analytic=cid.endswith("_analytic")))
        for x in hc.iterates(o.starting_point()):
            for sigma, lam in hc.draws(o.m) + [(-1.3, np.linspace(-2, 2, o.m))]:
                h, mag = o.eval_h(x, sigma, lam), o.eval_h_mag(x, sigma, lam)
                assert np.all(np.isfinite(mag)) and np.all(mag >= 0)
                assert np.all(mag >= np.abs(h))                       # hence mag == 0 only where H == 0
                assert np.all(h[mag == 0] == 0)
                assert np.array_equal(mag, o.eval_h_mag(x, -sigma, lam))
                assert np.array_equal(mag, o.eval_h_mag(x, sigma, -lam))
                flip = np.where(np.arange(o.m) % 3 == 0, -lam, lam)
                assert np.array_equal(mag, o.eval_h_mag(x, sigma, flip))
        # every stored entry that depends on anything at all has a magnitude: a zero multiplier vector and sigma = 0 give 0
        assert not np.any(o.eval_h_mag(x, 0.0, np.zeros(o.m)))


@pytest.fixture(scope="module")
def measured(built, tmp_path_factory):
    """c_ref and the resolved share per (case, step): strict build against the FMA build of the same sources."""
    fma = orc.build_variant(str(tmp_path_factory.mktemp("oracle_fma")), orc.FMA_CFLAGS)
    out = {}
    for cid, name, make in ALL:
        an = cid.endswith("_analytic")
        for step in hc.STEPS:
            prob, opts = make(), hc.exact_options(step, analytic=an)
            a, b = orc.Oracle(prob, opts), orc.Oracle(prob, opts, library=fma)
            c_ref, n_ok, n_nz = 0.0, 0, 0
            for x in hc.iterates(a.starting_point()):
                for sigma, lam in hc.draws(a.m):
                    h, mag = a.eval_h(x, sigma, lam), a.eval_h_mag(x, sigma, lam)
                    c_ref = max(c_ref, hc.noise_ratio(b.eval_h(x, sigma, lam), h, mag))
                    nz = h != 0
                    n_nz += int(nz.sum())
                    n_ok += int(np.sum(hc.C_NOISE * hc.EPS * mag[nz] <= hc.RESOLVED_RTOL * np.abs(h[nz])))
            out[(cid, step)] = (c_ref, n_ok / max(n_nz, 1))
    return out


def test_noise_constant_covers_two_builds_of_the_oracle(measured):
    worst = max(measured, key=lambda k: measured[k][0])
    c_ref = measured[worst][0]
    print("c_ref per case:", {"%s@%g" % k: round(v[0], 4) for k, v in measured.items()})
    assert 8.0 * c_ref <= hc.C_NOISE, (worst, c_ref)


@pytest.mark.parametrize("cid", ALL_IDS)
def test_coarse_step_resolves_most_of_every_case(measured, cid):
    c_ref, share = measured[(cid, 1e-3)]
    assert share >= hc.RESOLVED_SHARE, share


def test_committed_profile_states_the_same_constant(measured):
    with open(os.path.join(HERE, "..", "profiles", "hessian_noise.json")) as f:
        prof = json.load(f)
    assert prof["C"] == hc.C_NOISE
    assert sorted(prof["c_ref"]) == sorted("%s@%g" % (cid, step) for cid in ALL_IDS for step in hc.STEPS)
    assert 8.0 * max(prof["c_ref"].values()) <= prof["C"] == 2.0 ** np.ceil(np.log2(8.0 * max(max(prof["c_ref"].values()), 1.0)))
    for (cid, step), (c_ref, _) in measured.items():       # the file says what the oracle gives (it keeps 4 digits)
        assert abs(prof["c_ref"]["%s@%g" % (cid, step)] - c_ref) <= 1e-3 * c_ref, (cid, step, c_ref)
