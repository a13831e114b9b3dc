"""Power-posterior (heated) chains on the MI355X: the identities of tests/test_power_posterior.py through the product
libraries -- k_sweep_heated, the locus-rate scan, the decision stages of k_global -- at the goldens' own sizes.

A, B and D on m3 (migration bands, SPR traffic) and v8 (locus-mut-rate VAR), C on a7 (an estimated sample age); bit for bit,
no tolerance (power_posterior_util.py says why the chains must be equal).  F: the marginal-likelihood ladder of the program
against the quadrature, once."""
import pytest

import power_posterior_util as U

pytestmark = pytest.mark.gpu
_runs = {}


def chains(name):
    if name not in _runs:
        iters = U.FIXTURES[name][0]
        p = U.load(name)
        d = U.scaled_counts(p, 2)
        _runs[name] = dict(pack=p, one=U.run(None, p, iters), dbl=U.run(None, d, iters), dbl_half=U.run(None, d, iters, beta=0.5),
                           two=U.run(None, p, iters, beta=2.0))
    return _runs[name]


@pytest.mark.parametrize("name", ["m3", "v8"])
def test_fixture_covers_its_proposals(name):
    r = chains(name)
    iters, kinds = U.FIXTURES[name]
    U.covered(r["pack"], iters, r["one"], kinds)
    assert r["one"]["accept"] != r["dbl"]["accept"]


@pytest.mark.parametrize("name", ["m3", "v8"])
def test_a_half_on_doubled_counts(name):
    r = chains(name)
    U.same_chain(r["one"], r["dbl_half"])
    U.data_scaled(r["one"], r["dbl_half"], 2.0)


@pytest.mark.parametrize("name", ["m3", "v8"])
def test_b_two_on_the_pack(name):
    r = chains(name)
    U.same_chain(r["dbl"], r["two"])
    U.data_scaled(r["two"], r["dbl"], 2.0)


def test_c_zero_is_the_prior():
    name, (iters, kinds) = "a7", U.FIXTURES["a7"]
    p = U.load(name)
    one = U.run(None, p, iters)
    U.covered(p, iters, one, kinds)
    blank = U.run(None, U.scaled_counts(p, 0), iters)
    zero = U.run(None, p, iters, beta=0.0)
    assert blank["dataLogLikelihood"] == 0.0 and not blank["treeDataLnL"].any()
    U.same_chain(blank, zero)
    assert zero["dataLogLikelihood"] != 0.0 and zero["accept"] != one["accept"]


@pytest.mark.parametrize("name", ["m3", "v8"])
def test_d_beta_one_changes_nothing(name, tmp_path):
    iters = U.FIXTURES[name][0]
    p = chains(name)["pack"]
    plain = U.run(None, p, iters, dump=str(tmp_path / "plain.state"))
    before = U.run(None, p, iters, beta=1.0, dump=str(tmp_path / "before.state"))
    midrun = U.run(None, p, iters, beta=1.0, beta_from=iters // 2, dump=str(tmp_path / "midrun.state"))
    want = (tmp_path / "plain.state").read_bytes()
    assert len(want) > 1000
    assert (tmp_path / "before.state").read_bytes() == want and (tmp_path / "midrun.state").read_bytes() == want
    for r in (before, midrun):
        U.same_chain(plain, r)
        U.data_scaled(plain, r, 1.0)


def test_f_estimates_against_quadrature(tmp_path):
    """the ladder of tests/test_marginal_likelihood.py at the same sizes (K = 16, b = 100, s = 400: launch-bound at six loci,
    a few seconds), so with the tolerance derived there: the host build runs the same code"""
    import gphocs_amd as G
    from test_marginal_likelihood import ML, SD_SS, SD_TI, check_estimates
    fine, coarse = U.toy_lnZ(1e-4, 2e-4), U.toy_lnZ(2e-4, 4e-4)
    check_estimates(G.load_library(dims=(2, 3, 0)), tmp_path, (fine, abs(fine - coarse)), ML["s"], SD_SS, SD_TI)
