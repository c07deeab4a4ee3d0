"""GPU: the four deriv / marginal / expectation drivers of plk_engine.hip keep their integer tables, matrix streams and
workspace in grow-only engine buffers (d_u4pack, d_u4tip, d_uvmat, d_work) that every query of every driver writes
anew.  A query must therefore give the same bits whatever ran on the engine before it, also after a larger model left
the buffers longer than the next one needs.

The sequence, on one engine, under forced site chunking: plk_deriv with an edge mask, plk_edge_pair_sums,
plk_mixture_sens, plk_marginal with a node mask, the site-summed plk_marginal (per-wave sums in the specialised drivers).
Each result is compared bit for bit (np.array_equal on the doubles) with the same query on a fresh engine that ran
nothing before it.

test_generic_sequence: PLK_OPT_FORCE_GENERIC = 1, PLK_OPT_SITE_CHUNK = 64 (GEN_BLOCK), S = 200: four chunks, the last one
of 8 sites.  5-taxon rooted binary trees (E = 8).  First k = 61, C = 3 (K = 61): one padded matrix stream is
C E K K = 89 304 doubles, 24 past a multiple of 32, so the second and third stream of d_uvmat start where the driver
rounds them to, not where the first one ends; then, on the same engine, k = 3, C = 2 (K = 4), whose tables and streams
take a fraction of the retained buffers.  Every result is also held against the oracle at the bars of the generic-path
tests: deriv 1e-12 of the row scale and marginal 1e-12 per site, 1e-13 sum_s |w_s| v_s (+ 1e-15 sum_s |w_s| for marginals)
for their site sums (tests/test_gpu_kernel_families.py); W and the root rows 1e-12 of max|.| per (category, edge)
(tests/test_gpu_pair_sums.py); prior_out and rate_out 1e-12 of max_c |.| (tests/test_gpu_query_variants.py).
The 200 sites show P = 5 patterns, site s pattern s mod 5 (64 is no multiple of 5: every chunk starts at another
pattern), so the oracle runs on 5 sites and the sums are its per-pattern values under the pattern counts, exactly
(the aggregation of test_gpu_query_variants._second_pass).  W is the oracle's binary128 one at both state counts.  The
k = 61 reference is what this test costs: the oracle's binary128 exponentials for the mixture and for the three
one-category models of mixsens_cases.expectations, prepared once each, and W; the engines are set up without them.

test_specialised_sequence: the same sequence, twice round, on the driver the engine picks for k = 4 compact codes
(run_updown4, UD4_BLOCK = 256), k = 20 (run_updown_vec, UDV_BLOCK = 128) and k = 61 (run_updown_mfma, MF_SITES = 64);
there pair sums and the mixture gradient of k = 20 and 61 run on the generic driver in between, on the same buffers.  A
forced chunk of 64 is rounded up to one tile by the first two, so S is the smallest count that still makes three
chunks: 2 tiles + 1 (513, 257), and 200 for the matrix-core driver."""
import numpy as np
import pytest

import mixsens_cases
import qgrad_cases
from helpers import custom_workload, numeric_divisor_doc
from phyly_amd import engine as E_
from test_gpu_kernel_families import PROB_ULP, SUM_TOL, TOL, _row_err
from test_gpu_pair_sums import _check
from test_gpu_query_variants import _check_mixture, _ld, _wsum

pytestmark = pytest.mark.gpu
LD = np.longdouble

S_GENERIC, CHUNK, P = 200, 64, 5
TAXA = 5
STEPS = ("deriv", "pair_sums", "mixture_sens", "marginal", "marginal_sums")
GENERIC, K4, MFMA, VEC = 2, 1, 3, 4


def _workload(k):
    C = {3: 2, 4: 2, 20: 2, 61: 3}[k]
    wl = custom_workload(k, TAXA, C=C, root="custom" if k != 20 else "uniform", seed=5200 + k)
    assert wl.E == 2 * TAXA - 2 and all(wl.indptr[a + 1] - wl.indptr[a] in (0, 2) for a in range(wl.N))      # rooted, binary
    return wl


class _Case:
    """a model with S sites of P patterns; with an oracle, its per-pattern reference values"""

    def __init__(self, k, S, oracle=None):
        self.k, self.S = k, S
        self.wl = wl = _workload(k)
        self.pats = np.concatenate([wl.simulate(P - 2), wl.random_codes(2, seed=k, missing_frac=0.1)], axis=1)
        self.site_pat = np.arange(S) % P
        self.codes = np.ascontiguousarray(self.pats[:, self.site_pat])
        self.doc = numeric_divisor_doc(wl, self.pats)
        self.emask = np.array([(e * 5 + 1) % 3 != 0 for e in range(wl.E)], dtype=np.int32)
        self.nmask = (np.arange(wl.N) % 3 != 1).astype(np.int32)
        self.engine_model = None
        if oracle is None:
            return
        precise = 2 if k <= 8 else 1
        self.count = np.bincount(self.site_pat, minlength=P).astype(LD)
        m = oracle.parse_model(self.doc)
        w = oracle.prepare(m)
        self.deriv = oracle.site_deriv(m, w, m.B, precise=precise)
        self.marg = oracle.site_marginal(m, w, m.B, precise=precise)
        self.W = qgrad_cases.oracle_W_factored(oracle, m, w, None)
        self.R = qgrad_cases.oracle_root(oracle, m, w, None, per_category=True)
        self.mix = mixsens_cases.expectations(oracle, self.doc, self.count, cache={("model", "mixture"): (m, w)})

    def setup(self, eng, oracle, options):
        """mixsens_cases.setup_engine (the document's tree and model through the product's own K0) without the oracle's
        prepared workspace, which the engine does not need and which takes seconds at k = 61"""
        for o, v in options.items():
            eng.set_option(o, v)
        if self.engine_model is None:
            m = oracle.parse_model(self.doc)
            self.engine_model = (m, mixsens_cases.product_k0(m))
        m, k0 = self.engine_model
        assert m.root_mode in (E_.ROOT_CUSTOM, E_.ROOT_UNIFORM)
        rw = np.asarray(m.root_custom, dtype=float) if m.root_mode == E_.ROOT_CUSTOM else None
        eng.set_tree(m.indptr, m.indices, m.preorder)
        eng.set_model(k0["Qn"], m.edge_rates_csr, k0["cat_rates"], k0["cat_prior"], m.root_mode, rw, Qn_lo=k0["Qn_lo"])
        eng.set_patterns_codes(self.codes, self.wl.defs)

    def run(self, eng, step):
        """-> (the arrays the query returns, (up/down kernel, pair-sum kernel, mixture-gradient kernel) it reports)"""
        if step == "deriv":
            out = eng.deriv(edge_mask=self.emask)
        elif step == "pair_sums":
            out = eng.edge_pair_sums()
        elif step == "mixture_sens":
            out = eng.mixture_sens()
        elif step == "marginal":
            out = eng.marginal(node_mask=self.nmask)
        else:
            out = eng.marginal(per_site=False)[1:]
        return out, (eng.info(E_.INFO_UPDOWN_KERNEL), eng.info(E_.INFO_PAIR_SUMS_KERNEL), eng.info(E_.INFO_MIXTURE_SENS_KERNEL))

    def check_oracle(self, step, out, tag):
        esel, nsel = self.emask.astype(bool), self.nmask.astype(bool)
        ones = np.ones(self.S)
        if step == "deriv":
            got, sums = out
            want = self.deriv[self.site_pat]
            assert _row_err(got[:, esel], want[:, esel]) <= TOL, tag
            assert np.all(got[:, ~esel] == 0.0) and np.all(sums[~esel] == 0.0), tag
            bound = SUM_TOL * np.sum(np.max(np.abs(want), axis=1))
            ref_sum = np.tensordot(self.count, np.asarray(self.deriv, dtype=LD), axes=(0, 0))
            assert np.max(np.abs(_ld(sums)[esel] - ref_sum[esel])) <= bound, tag
        elif step == "pair_sums":
            _check(tag + " W", _ld(out[0]), _wsum(self.W, self.count), 1e-12)
            _check(tag + " root", _ld(out[1]), _wsum(self.R, self.count), 1e-12)
        elif step == "mixture_sens":
            _check_mixture(tag, out[0], out[1], self.mix)
        else:
            sums = out[-1]
            want = self.marg[self.site_pat]
            ref_sum = np.tensordot(self.count, np.asarray(self.marg, dtype=LD), axes=(0, 0))
            bound = SUM_TOL * np.tensordot(self.count, np.abs(np.asarray(self.marg, dtype=LD)), axes=(0, 0)) + PROB_ULP * np.sum(ones)
            if step == "marginal":
                assert np.max(np.abs(out[0][:, nsel] - want[:, nsel])) <= TOL, tag
                assert np.all(out[0][:, ~nsel] == 0.0) and np.all(sums[~nsel] == 0.0), tag
                assert np.all(np.abs(_ld(sums) - ref_sum)[nsel] <= bound[nsel]), tag
            else:
                assert np.all(np.abs(_ld(sums) - ref_sum) <= bound), tag


_CASES = {}


def _case(k, S, oracle=None):
    key = (k, S, oracle is not None)
    if key not in _CASES:
        _CASES[key] = _Case(k, S, oracle)
    return _CASES[key]


def _fresh(case, oracle, options, step):
    """the query on an engine that has run nothing else"""
    e = E_.Engine(0)
    try:
        case.setup(e, oracle, options)
        return case.run(e, step)
    finally:
        e.close()


def _same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_generic_sequence(oracle):
    options = {E_.OPT_FORCE_GENERIC: 1, E_.OPT_SITE_CHUNK: CHUNK}
    eng = E_.Engine(0)
    try:
        for k in (61, 3):
            case = _case(k, S_GENERIC, oracle)
            C, E, K = int(case.wl.prepare()["cat_rates"].shape[0]), case.wl.E, {61: 61, 3: 4}[k]
            assert (C, E) == ({61: 3, 3: 2}[k], 8) and (k != 61 or (C * E * K * K) % 32 == 24)
            case.setup(eng, oracle, options)
            for step in STEPS:
                tag = "generic k=%d %s" % (k, step)
                out, kernels = case.run(eng, step)
                want, _ = _fresh(case, oracle, options, step)
                assert kernels[{"pair_sums": 1, "mixture_sens": 2}.get(step, 0)] == GENERIC, tag
                assert _same_bits(out, want), tag
                case.check_oracle(step, out, tag)
    finally:
        eng.close()


@pytest.mark.parametrize("k,S,updown,sums", [(4, 513, K4, K4), (20, 257, VEC, GENERIC), (61, S_GENERIC, MFMA, GENERIC)],
                         ids=["k4", "vec", "mfma"])
def test_specialised_sequence(oracle, k, S, updown, sums):
    options = {E_.OPT_SITE_CHUNK: CHUNK}
    case = _case(k, S)
    fresh = {step: _fresh(case, oracle, options, step) for step in STEPS}
    eng = E_.Engine(0)
    try:
        case.setup(eng, oracle, options)
        for rnd in range(2):
            for step in STEPS:
                tag = "k=%d round %d %s" % (k, rnd, step)
                out, kernels = case.run(eng, step)
                assert kernels[{"pair_sums": 1, "mixture_sens": 2}.get(step, 0)] == (sums if step in ("pair_sums", "mixture_sens") else updown), tag
                assert _same_bits(out, fresh[step][0]), tag
    finally:
        eng.close()
