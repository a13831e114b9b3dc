"""Phase integration at the edges of its groups on the MI355X: the packs of phase_edges_util.py through the product libraries.

The host build's fiber wave emulates the lane shift of add_phases and cannot vouch for it; here the five device texts run:
add_phases behind lik_compute in its lane-per-node form (variants s, x), in its list-driven form (h, n), behind lik_private_t and
lr_ref_eval (locus-mut-rate VAR: v8, with locus 0 -- the scan's reference locus -- once the [64] layout and once P = 63 with a group
of 32), and root_sum_generic (the wide loci; with GPH_HUGE_LDS on a block in HBM).  Each run is compared with the oracle run live on
the same pack -- counters exact, sums <= 1e-10 relative, the final state with the conditionals field by field -- and with the
60-digit decimal model of the final gene trees (<= 1e-10 relative per locus; the deviations measured stand in the docstrings).
Identities A and B of test_power_posterior_gpu.py put k_sweep_heated, a second text of the same root reduction, on the same pack.
The refusals of gph_engine_load_loci go through a product library too: gph_engine_load_loci alone, nothing is launched."""
import copy
import os
import time

import pytest

from conftest import REPO
from parity_util import compare_records, compare_states
import phase_edges_util as U
import power_posterior_util as PP

pytestmark = pytest.mark.gpu

# id: (model, library variant load_library(dims=...) must pick, layout that becomes locus 0, a count of 70000, iterations)
CASES = {
    "m3": ("m3", "s", 0, False, 30),
    "v8-ref64": ("v8", "s", U.I_64, False, 30),
    "v8-ref63": ("v8", "s", U.I_P63, False, 30),
    "x8": ("x8", "x", 0, True, 24),
    "y9": ("y9", "h", 0, False, 30),
    "n7": ("n7", "n", 0, False, 20),
}
OVERRIDES = {"lds-sum-0": {"GPH_LDS_SUM": "0"}, "lds-sum-1": {"GPH_LDS_SUM": "1"}, "huge-lds": {"GPH_HUGE_LDS": "5200"}, "cnt32": {"GPH_CNT16": "0"}}
_runs = {}


@pytest.fixture(scope="module")
def G():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import gphocs_amd as G
    G.build()
    return G


def chain(G, case, oracle_cli, tmp_path_factory):
    """the pack, the engine's run on the product library of its size and the oracle's, once per case"""
    if case not in _runs:
        from gphocs_amd_pkg import synth
        base, variant, first, big_count, iters = CASES[case]
        d = tmp_path_factory.mktemp(case)
        pack = U.narrow_pack(base, big_count=big_count, first=first)
        assert G.variant_for(pack.n, pack.K, pack.B) == variant
        path = str(d / "pack.gpk")
        synth.write_pack(pack, path)
        f = {k: str(d / k) for k in ("e.trace", "e.state", "o.trace", "o.state")}
        t0 = time.time()
        r = U.run(G, G.load_library(dims=(pack.n, pack.K, pack.B)), G.Pack.load(path), iters, f["e.trace"], f["e.state"])
        t1 = time.time()
        U.run_oracle(oracle_cli, path, iters, f["o.trace"], f["o.state"])
        print(f"{case}: engine {t1 - t0:.2f} s, oracle {time.time() - t1:.2f} s")
        _runs[case] = dict(pack=pack, path=path, iters=iters, r=r, files=f, dir=d)
    return _runs[case]


@pytest.mark.parametrize("case", sorted(CASES))
def test_against_live_oracle(G, case, oracle_cli, tmp_path_factory):
    c = chain(G, case, oracle_cli, tmp_path_factory)
    U.covered(c["pack"], c["iters"], c["r"], U.kinds_for(c["pack"]))
    assert c["r"]["oob"] == (0, 0)
    f = c["files"]
    worst = compare_records(f["e.trace"], f["o.trace"])
    compare_states(f["e.state"], f["o.state"])
    print(f"{case}: worst accumulator deviation {worst:.3e}")


@pytest.mark.parametrize("case", sorted(CASES))
def test_against_decimal_model(G, case, oracle_cli, tmp_path_factory):
    """largest |device dataLnL - model| / |model| over the loci after the last iteration, as measured on the MI355X:
    m3 1.5e-15, v8-ref64 1.6e-15, v8-ref63 1.4e-14, x8 3.0e-15, y9 1.1e-14, n7 3.3e-14 -- the host builds' figures: the chains are the
    oracle's on both, and the per-locus values equal to the last bit"""
    c = chain(G, case, oracle_cli, tmp_path_factory)
    worst = U.model_deviation(c["pack"], c["r"])
    print(f"{case}: largest deviation from the decimal model {worst:.3e}")
    assert worst <= U.MODEL_TOL


@pytest.mark.parametrize("form", sorted(OVERRIDES))
def test_launch_forms(G, form, oracle_cli, tmp_path_factory, tmp_path, capfd):
    """the m3-model pack with the root sum's terms through LDS or by lane reads, with the 32-bit counts, and with the sequence
    blocks of the wide loci in HBM: the default run's records and state byte for byte, and the oracle's"""
    c = chain(G, "m3", oracle_cli, tmp_path_factory)
    pack = c["pack"]
    tr, st = str(tmp_path / "t"), str(tmp_path / "s")
    capfd.readouterr()
    r = U.run(G, G.load_library(dims=(pack.n, pack.K, pack.B)), G.Pack.load(c["path"]), c["iters"], tr, st, env=OVERRIDES[form])
    err = capfd.readouterr().err
    assert ("keep their sequence block in HBM" in err) == (form == "huge-lds"), err
    f = c["files"]
    compare_records(tr, f["o.trace"])
    compare_states(st, f["o.state"])
    assert open(tr).read() == open(f["e.trace"]).read()
    assert open(st).read() == open(f["e.state"]).read()
    assert r["accept"] == c["r"]["accept"]


@pytest.mark.parametrize("case,big", [("m3", False), ("y9", True)])
def test_checked_builds_find_no_index_out_of_range(G, case, big, oracle_cli, tmp_path_factory, tmp_path):
    """the libraries compiled with -DGPH_BOUNDS (capacities of variant x: lane-per-node; of variant b: list-driven) on the same
    packs: the oracle's results and no index out of range"""
    c = chain(G, case, oracle_cli, tmp_path_factory)
    chk = os.path.join(REPO, "g-phocs_amd", G.CHECKED_LIB_BIG if big else G.CHECKED_LIB)
    assert os.path.exists(chk)
    tr, st = str(tmp_path / "t"), str(tmp_path / "s")
    r = U.run(G, G.load_library(chk), G.Pack.load(c["path"]), c["iters"], tr, st)
    assert r["oob"] == (0, 1)
    compare_records(tr, c["files"]["o.trace"])
    compare_states(st, c["files"]["o.state"])


def test_groups_of_2_to_the_14_and_15(G, oracle_cli, tmp_path):
    """phase words 16384 and 0x8000 | 15 (the smallest encoded word) on the wide path, sequence blocks in HBM, two iterations
    against the oracle.  Observed on the MI355X: 0.84 s for load, initialize and the two iterations"""
    from gphocs_amd_pkg import synth
    pack = U.huge_pack()
    assert sorted(set(pack.numPhases.tolist()))[-2:] == [16384, 0x8000 | 15]
    path = str(tmp_path / "k15.gpk")
    synth.write_pack(pack, path)
    f = {k: str(tmp_path / k) for k in ("e.trace", "e.state", "o.trace", "o.state")}
    t0 = time.time()
    r = U.run(G, G.load_library(dims=(pack.n, pack.K, pack.B)), G.Pack.load(path), 2, f["e.trace"], f["e.state"], with_cond=False)
    print(f"2^14 / 2^15: engine {time.time() - t0:.2f} s for initialize and two iterations")
    U.run_oracle(oracle_cli, path, 2, f["o.trace"], f["o.state"], with_cond=False)
    compare_records(f["e.trace"], f["o.trace"])
    compare_states(f["e.state"], f["o.state"])
    assert r["dataLogLikelihood"] < 0


# ---------------------------------------------------------------- identities A and B (power_posterior_util.py) on the m3-model pack
def heated(G):
    if "heated" not in _runs:
        p = U.narrow_pack("m3")
        d = PP.scaled_counts(p, 2)
        iters = CASES["m3"][4]
        _runs["heated"] = dict(pack=p, iters=iters, one=PP.run(None, p, iters), dbl=PP.run(None, d, iters),
                               dbl_half=PP.run(None, d, iters, beta=0.5), two=PP.run(None, p, iters, beta=2.0))
    return _runs["heated"]


def test_a_half_on_doubled_counts(G):
    r = heated(G)
    PP.covered(r["pack"], r["iters"], r["one"], ("coal", "spr", "tau", "mixing"))
    assert r["one"]["accept"] != r["dbl"]["accept"]
    PP.same_chain(r["one"], r["dbl_half"])
    PP.data_scaled(r["one"], r["dbl_half"], 2.0)


def test_b_two_on_the_pack(G):
    r = heated(G)
    PP.same_chain(r["dbl"], r["two"])
    PP.data_scaled(r["two"], r["dbl"], 2.0)


# ---------------------------------------------------------------- the load boundary through a product library
MALFORMED = sorted(U.malformed(U.m3()))


def test_refusals_through_a_product_library(G, capfd, tmp_path):
    """every malformed array of test_phase_edges.py and the size rule: gph_engine_load_loci alone, refused with the locus named;
    the same library then runs m3 to its golden's records"""
    from conftest import GOLDEN
    p = U.m3()
    lib = G.load_library(dims=(p.n, p.K, p.B))
    for what in MALFORMED:
        locus, pattern, code, change = U.malformed(p)[what]
        q = copy.deepcopy(p)
        change(q)
        U.check_refusal(lib, q, capfd, locus, code, pattern)
    U.check_refusal(lib, U.oversized(p), capfd, 1, -101)
    tr = str(tmp_path / "t")
    s = G.Sampler(p, lib=lib)
    s.set_record_file(tr)
    s.initialize()
    for it in range(12):
        s.iteration(it)
    s.set_record_file(None)
    s.close()
    # the first records of the golden's 120 iterations
    got = open(tr).read().splitlines()
    assert sum(x.startswith("IT") for x in got) >= 12
    (tmp_path / "want").write_text("\n".join(open(os.path.join(GOLDEN, "m3.rtrace")).read().splitlines()[:len(got)]) + "\n")
    compare_records(tr, str(tmp_path / "want"))
