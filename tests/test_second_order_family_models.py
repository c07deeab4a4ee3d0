"""CPU only: the data and the norm of tests/test_gpu_second_order_families.py can tell a wrong second-order pass from a
right one.

For each state count of second_order_cases.FAMILY_KS, on helpers.family_workload(k) (non-reversible Q, unequal category
priors, a rate-0 category, every root prior, data on internal nodes) with second_order_cases.conserved_codes:
- every site ll, derivative and Hessian of the oracle is finite at all three site counts of the GPU test, so that test
  leaves no site out;
- the long-double reference agrees with binary128 on its first sites to 1e-14 of the largest entry;
- every wrong kernel of second_order_cases.mutants that applies to the model moves the weighted Hessian by at least
  MOVES = 1e-6 in the scaled norm (or makes a site likelihood 0: NaN counts as moved); the ones that do not apply are
  named in NOT_APPLICABLE with the reason, and the table is held to what mutants() reports.
Also recorded: uniformly random codes, which the earlier Hessian cases use, fail the edge-swap condition at k = 20."""
import numpy as np
import pytest

from helpers import family_workload, oracle_model
import second_order_cases as cases

S, SEED = 65, 65
SWAP, ROLL, QT, PT, ROOT, INNER = cases.MUTANTS

# mutants that cannot apply, by model
NOT_APPLICABLE = {
    2: {ROOT, INNER},                 # root prior none, data at the leaves only
    5: set(),
    9: {ROOT, INNER},                 # uniform root prior
    13: {ROLL},                       # four gamma categories of equal prior, no rate-0 category
    20: set(),
    27: {ROOT},                       # root prior none
    33: {INNER},
    48: {ROLL, ROOT},                 # two categories of equal prior; root prior none
    61: {ROLL, INNER},                # two categories of equal prior
}


def _moved(err):
    return np.isnan(err) or err >= cases.MOVES


def _model(oracle, k, codes_of):
    wl = family_workload(k)
    codes = codes_of(wl)
    m, w = oracle_model(oracle, wl, codes)
    return wl, codes, m, w


@pytest.mark.parametrize("k", cases.FAMILY_KS)
def test_no_site_is_left_out(oracle, k):
    """the finiteness condition at the three site counts, and the long double against binary128 check on each"""
    wl = family_workload(k)
    m = w = None
    for size in cases.FAMILY_SIZES:
        codes = cases.conserved_codes(wl, size, size)
        assert codes.shape == (wl.N, size) and codes.dtype == np.uint8 and codes.max() < wl.nchar
        if m is None:
            m, w = oracle_model(oracle, wl, codes)
        ref = cases.Reference(oracle, m, w, wl.defs[codes.T])       # asserts both
        assert ref.finite and ref.ld_gap <= 1e-14, (size, ref.ld_gap)
        assert ref.H.shape == (size, wl.E, wl.E)
        _, _, d, _ = ref.sums()
        assert np.all(d > 0), size                                   # every edge has a scale of its own: (b) divides by it


@pytest.mark.parametrize("k", cases.FAMILY_KS)
def test_mutants_move_the_scaled_norm(oracle, k):
    wl, codes, m, w = _model(oracle, k, lambda wl: cases.conserved_codes(wl, S, SEED))
    wts = np.linspace(0.5, 1.5, S)
    ref = cases.Reference(oracle, m, w, wl.defs[codes.T])
    _, H, d, _ = ref.sums(wts)
    ratio = np.max(np.abs(H) / np.outer(d, d))
    assert 0.25 <= ratio <= 1.0, ratio                               # the scale is neither slack nor tight
    muts = cases.mutants(wl, m, w, codes)
    assert tuple(muts) == cases.MUTANTS
    assert {name for name, v in muts.items() if isinstance(v, str)} == NOT_APPLICABLE[k]
    for name, v in muts.items():
        if isinstance(v, str):
            continue
        wm, cm = v
        err = cases.scaled_err(cases.weighted_hess(oracle, m, wm, wl.defs[cm.T], wts), H, d)
        print("k=%d %s: scaled err %.3g" % (k, name, err))
        assert _moved(err), (k, name, err)


def test_every_mutant_applies_somewhere():
    for name in cases.MUTANTS:
        assert any(name not in NOT_APPLICABLE[k] for k in cases.FAMILY_KS), name


def test_random_codes_hide_the_rate_categories(oracle):
    """why the data are conserved: with uniformly random codes at k = 20 the fastest category carries the site
    likelihoods, and categories swapped on the edge of largest rate do not move the Hessian by MOVES"""
    wl, codes, m, w = _model(oracle, 20, lambda wl: wl.random_codes(S, seed=SEED, missing_frac=0.1))
    wts = np.linspace(0.5, 1.5, S)
    Hs = oracle.site_hess(m, w, wl.defs[codes.T], precise=1)
    gs = oracle.site_deriv(m, w, wl.defs[codes.T], precise=1)
    assert np.all(np.isfinite(Hs))
    H = (Hs * wts[:, None, None]).sum(axis=0)
    d = cases.edge_scale(Hs, gs, wts)
    wm, cm = cases.mutants(wl, m, w, codes)[SWAP]
    err = cases.scaled_err(cases.weighted_hess(oracle, m, wm, wl.defs[cm.T], wts), H, d)
    assert err < cases.MOVES, err
