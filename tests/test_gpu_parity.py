"""GPU parity tests (-m gpu): the HIP path, called through the C ABI (ctypes), against
 (a) the committed golden vectors generated from the REAL reference, and
 (b) the oracle restatement run live on the same seeded inputs.
Accept/reject counters of every proposal in every iteration must be identical; accumulators (sums over
loci) within 1e-10 relative; the full per-locus state -- topology, event chains with ids and lineage
counts, statistics, RNG slots, ages, elapsed times, conditionals, per-locus log-likelihoods -- BYTE FOR BYTE
(parity_util.STATE_TOL = 0).  Trace files of the program: every parameter column character-identical to the
real binary's, the two log-likelihood columns within 1e-10 relative (parity_util.compare_trace_files)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO
from parity_util import compare_records, compare_states, compare_trace_files

pytestmark = pytest.mark.gpu

CASES = {"g1": 30, "g2": 30, "m3": 120, "m4": 60, "c5": 30, "s3": 40, "a6": 80, "a7": 100, "z0": 12, "v8": 60, "v9": 60,
         "w2": 50,   # w2: model from a primary + a secondary control file
         "r5": 60,   # r5: locus-mut-rate FIXED <rate file> (readRateFile, GPhoCS.c:491-579): per-locus rates 0.2 .. 5 before normalisation
         "x8": 24,   # x8: 32 leaves, 31 populations, 16 bands: the largest lane-per-node build (library variant x)
         "y9": 16,   # y9: 40 leaves, 39 populations (the reference's NSPECIES cap), 16 bands: library variant h
         "n7": 12,   # n7: 72 leaves: library variant n (200 leaves / 39 populations / 100 bands, the reference's own caps)
         "q6": 8,    # q6: 72 leaves, two 20-kb loci with 145 and 698 phased patterns (up to 512 phases): the second one's sequence block (28 KB) lies beyond the LDS budget next to variant n's 44-KB image and stays in HBM
         # round 6: population trees that are not caterpillars, migration bands with ancestral endpoints (the band-start branches of
         # UpdateTau, GPhoCS.c:3353-3431; tau bounds from two ancestral sons, :3266-3267; rubberBandRipple with start_or_end == 1)
         "j1": 150,  # (((A,B),(C,D)),E), bands AB->CD, CD->AB, C->AB, E->ABCD
         "j2": 100,  # ((A,(B,C)),((D,E),F)), 8 bands: leaf<->ancestral, ancestral<->ancestral, leaf->leaf, D->BC across the root
         "j3": 120,  # ((A,B),(C,D)) with an ESTIMATED ancient sample in C under the band target CD
         "k3": 24,   # k3: the pack, records and states of a control file with burn-in 13 / mcmc-sample-skip 2 (test_program_trace_file runs its burn-in)
         "b2": 24}   # b2: 20 migration bands: library variant b (live-band list in LDS, model read from HBM, 384-column reduced rows)


@pytest.fixture(scope="module")
def G():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import gphocs_amd as G
    G.build()
    return G


NOCOND = {"q6"}      # goldens whose state dumps carry no conditional arrays (4 MB of hex floats for q6's 698 patterns x 71 nodes)


def _run(G, pack, iters, tmp_path, tag):
    s = G.Sampler(G.Pack.load(pack))
    tr, st0, st1 = tmp_path / f"{tag}.trace", tmp_path / f"{tag}.init.state", tmp_path / f"{tag}.state"
    s.set_record_file(str(tr))
    s.initialize()
    s.dump_state(str(st0), tag not in NOCOND)
    for it in range(iters):
        s.iteration(it)
    s.dump_state(str(st1), tag not in NOCOND)
    s.set_record_file(None)
    cnt = s.counters()
    s.close()
    return tr, st0, st1, cnt


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_reference_goldens(G, name, tmp_path):
    it = CASES[name]
    tr, st0, st1, cnt = _run(G, os.path.join(GOLDEN, name + ".gpk"), it, tmp_path, name)
    compare_states(st0, os.path.join(GOLDEN, name + ".init.state"))
    worst = compare_records(tr, os.path.join(GOLDEN, name + ".rtrace"))
    compare_states(st1, os.path.join(GOLDEN, name + ".state"))
    assert cnt["evals"] > 0
    print(f"{name}: worst accumulator rel diff {worst:.3e}, evals {cnt['evals']}")


@pytest.mark.parametrize("variant", ["l", "m", "x", "g", "h", "b", "n"])
@pytest.mark.parametrize("name", ["j1", "j2", "j3"])
def test_new_model_shapes_on_every_capacity_variant(G, name, variant, tmp_path):
    """round 6: the goldens with balanced / mixed population trees and ancestral band ends fit the smallest library (variant s or
    m), so the lane-per-node forms of 32 leaves (x), the list-driven multi-word forms of the big-tree builds (g, h), the
    many-band forms (b: live-band list in LDS, model read from HBM) and the reference's own caps (n) would never meet a band that
    starts above its target population's age.  Each variant is loaded explicitly and must reproduce the real reference's records
    and per-locus state (variant s / m run them in test_against_reference_goldens)."""
    pk = G.Pack.load(os.path.join(GOLDEN, name + ".gpk"))
    cl, ck, cb = G.VARIANTS[variant][:3]
    if pk.n > cl or pk.K > ck or pk.B > cb:
        pytest.skip(f"{name} ({pk.n} leaves, {pk.K} populations, {pk.B} bands) does not fit variant {variant}")
    lib = G.load_library(G.lib_path(variant))
    it = CASES[name]
    s = G.Sampler(pk, lib=lib)
    tr, st = tmp_path / "t", tmp_path / "s"
    s.set_record_file(str(tr))
    s.initialize()
    for k in range(it):
        s.iteration(k)
    s.dump_state(str(st), True)
    s.set_record_file(None)
    s.close()
    compare_records(tr, os.path.join(GOLDEN, name + ".rtrace"))
    compare_states(st, os.path.join(GOLDEN, name + ".state"))


def test_against_live_oracle(G, oracle_cli, tmp_path):
    """a case that is NOT a committed fixture length: 77 iterations of m4 vs the oracle run live"""
    pack = os.path.join(GOLDEN, "m4.gpk")
    tr, _, st1, _ = _run(G, pack, 77, tmp_path, "m4")
    ot, os_ = tmp_path / "o.trace", tmp_path / "o.state"
    subprocess.run([oracle_cli, "run", pack, "77", str(ot), str(os_), "76", "1"], check=True, timeout=600)
    compare_records(tr, ot)
    compare_states(st1, os_)


def test_many_patterns_against_live_oracle(G, oracle_cli, tmp_path):
    """loci with up to 75 phased patterns (more than one wavefront of (pattern, base) pairs and more
    than 64 per-pattern terms: exercises the multi-pass pruning and the LDS fallback of the root sum)"""
    pack = os.path.join(GOLDEN, "bigp.gpk")
    tr, _, st1, _ = _run(G, pack, 40, tmp_path, "bigp")
    ot, os_ = tmp_path / "o.trace", tmp_path / "o.state"
    subprocess.run([oracle_cli, "run", pack, "40", str(ot), str(os_), "39", "1"], check=True, timeout=600)
    compare_records(tr, ot)
    compare_states(st1, os_)


@pytest.mark.parametrize("config,loci,iters,mut,mig_beta", [(4, 3000, 24, 6.5, 1e-5), (5, 1500, 20, 3.0, 1e-5),
                                                             (3, 2000, 30, 1.0, 1e-5), (6, 1500, 24, 2.0, 4e-8),
                                                             (7, 1500, 24, 2.0, 4e-8), (4, 1500, 16, 3.0, 4e-8),
                                                             (4, 600, 400, 3.0, 4e-8),    # long trajectory
                                                             (10, 500, 12, 3.0, 4e-8),    # 40 leaves: library variant h
                                                             (11, 800, 16, 3.0, 4e-8),    # 23 populations, 6 bands: variant x
                                                             (12, 400, 16, 3.0, 4e-8),    # 20 migration bands: variant b
                                                             (13, 100, 10, 2.0, 1e-5),    # 72 leaves: variant n
                                                             (14, 30, 8, 0.5, 1e-5)])     # 136 leaves, 132 lineages in one population: variant n, lineage counts > 127
def test_scale_parity_against_live_oracle(G, oracle_cli, tmp_path, config, loci, iters, mut, mig_beta):
    """thousands of loci of the benchmark's synthetic shape (configs[3] and [4], the 3-population one, the two
    estimated-sample-age ones and a high-migration prior: mig-rate-beta 4e-8 puts thousands of migration events
    into the genealogies), through every proposal type, against the oracle run live on the same pack: ~10^5
    locus-iterations, so rare paths (migration-event creation and removal, rubber-band conflicts of UpdateTau and
    UpdateSampleAge, "not enough migration slots", checkAll resync at samples-per-log) are hit.  Counters exact, accumulators <= 1e-10 relative, final per-locus state field by field."""
    from gphocs_amd_pkg import synth
    pk = synth.make_synthetic_pack(G.Pack, config, loci, mut_scale=mut, data_seed=777 + config, mcmc_seed=4242,
                                   samples_per_log=8, mig_beta=mig_beta)
    pth = str(tmp_path / "scale.gpk")
    synth.write_pack(pk, pth)
    tr, _, st1, cnt = _run(G, pth, iters, tmp_path, "scale")
    ot, os_ = tmp_path / "o.trace", tmp_path / "o.state"
    subprocess.run([oracle_cli, "run", pth, str(iters), str(ot), str(os_), str(iters - 1), "0"], check=True,
                   timeout=1200)
    worst = compare_records(tr, ot)
    # state without conditionals on the oracle side: compare the genealogy / chain / statistics fields
    st_nc = tmp_path / "scale.nc.state"
    s = G.Sampler(G.Pack.load(pth))
    s.initialize()
    for it in range(iters):
        s.iteration(it)
    s.dump_state(str(st_nc), False)
    s.close()
    compare_states(st_nc, os_)
    print(f"config {config}: {loci} loci x {iters} iterations, worst accumulator rel diff {worst:.3e}, evals {cnt['evals']}")


@pytest.mark.parametrize("config,loci,iters,mut,alpha,ft,seqlen,pscr", [
    (3, 2000, 20, 1.0, 1.0, 0.3, 1000, None), (4, 1200, 16, 6.5, 1.6, 1.2, 1000, None),
    (2, 1500, 16, 14.0, 0.7, 0.6, 1000, None),
    (4, 400, 10, 24.0, 1.6, 1.2, 3000, None),    # loci with more than 64 phased patterns: strided path, LDS scratch
    (4, 400, 10, 24.0, 1.6, 1.2, 3000, "30")])   # ... and conditionals scratch in global memory beyond 30 patterns
def test_locus_rate_scale_parity_against_live_oracle(G, oracle_cli, tmp_path, monkeypatch, config, loci, iters, mut,
                                                     alpha, ft, seqlen, pscr):
    """`locus-mut-rate VAR`: UpdateLocusRate (one wavefront scanning the loci in order + parallel write-back) over
    thousands of loci against the oracle's serial loop on the same pack: small and large steps (reflections at both
    ends of (0, rold + rref)), alpha != 1 (Dirichlet prior term), pattern-rich loci (mut 14: loci with more than 64
    phased patterns take the strided path and, beyond the LDS scratch, the global scratch).  Counters exact,
    accumulators <= 1e-10 relative, per-locus state (rates included) field by field."""
    from gphocs_amd_pkg import synth
    if pscr:
        monkeypatch.setenv("GPH_LR_PSCR", pscr)
    pk = synth.make_synthetic_pack(G.Pack, config, loci, seqlen=seqlen, mut_scale=mut, data_seed=900 + config,
                                   mcmc_seed=777, samples_per_log=8)
    synth.make_var_rates(pk, alpha, ft)
    pth = str(tmp_path / "var.gpk")
    synth.write_pack(pk, pth)
    s = G.Sampler(G.Pack.load(pth))
    tr, st1 = tmp_path / "var.trace", tmp_path / "var.state"
    s.set_record_file(str(tr))
    s.initialize()
    for it in range(iters):
        s.iteration(it)
    s.dump_state(str(st1), False)
    s.set_record_file(None)
    s.close()
    ot, os_ = tmp_path / "o.trace", tmp_path / "o.state"
    subprocess.run([oracle_cli, "run", pth, str(iters), str(ot), str(os_), str(iters - 1), "0"], check=True,
                   timeout=1200)
    worst = compare_records(tr, ot)
    compare_states(st1, os_)
    nacc = sum(int(l.split()[3]) for l in open(tr) if " LRATE " in l)
    assert 0 < nacc < (loci - 1) * iters
    print(f"VAR config {config}: {loci} loci x {iters} iterations, {nacc} accepted rate moves, Pmax {int(np.diff(pk.pattern_offsets).max())}, worst rel diff {worst:.3e}")


@pytest.mark.parametrize("loci,zero_ref", [(1, False), (2, False), (70, False), (70, True)])
def test_locus_rate_edge_cases(G, oracle_cli, tmp_path, loci, zero_ref):
    """UpdateLocusRate with only the reference locus, with one proposing locus, across a batch boundary of the scan (65+
    loci), and with a reference locus without informative columns (P = 0), against the oracle run live."""
    from gphocs_amd_pkg import synth
    pk = synth.make_synthetic_pack(G.Pack, 3, loci, mut_scale=1.0, data_seed=5, mcmc_seed=99, samples_per_log=4)
    synth.make_var_rates(pk, 1.3, 0.8)
    if zero_ref:
        p0 = int(pk.pattern_offsets[1])
        pk.leafcodes, pk.numPhases, pk.counts = pk.leafcodes[p0:], pk.numPhases[p0:], pk.counts[p0:]
        pk.pattern_offsets = np.concatenate([[0], pk.pattern_offsets[1:] - p0]).astype(np.int64)
    pth = str(tmp_path / "ve.gpk")
    synth.write_pack(pk, pth)
    tr, _, st1, _ = _run(G, pth, 12, tmp_path, "ve")
    ot, os_ = tmp_path / "o.trace", tmp_path / "o.state"
    subprocess.run([oracle_cli, "run", pth, "12", str(ot), str(os_), "11", "1"], check=True, timeout=300)
    assert compare_records(tr, ot) <= 1e-10
    compare_states(st1, os_)


WORKER = r'''
import os, sys
sys.path.insert(0, %(repo)r)
import numpy as np, torch, torch.distributed as dist
import gphocs_amd as G
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
def allreduce(sums, mins):
    if sums.size:
        t = torch.from_numpy(sums); dist.all_reduce(t, op=dist.ReduceOp.SUM)
    if mins.size:
        t = torch.from_numpy(mins); dist.all_reduce(t, op=dist.ReduceOp.MIN)
s = G.Sampler(G.Pack.load(%(pack)r), device=0, rank=rank, world=world, allreduce=allreduce)
s.set_record_file(%(out)r + ".%%d" %% rank)
s.initialize()
for it in range(%(iters)d):
    s.iteration(it)
s.set_record_file(None)
s.close()
dist.destroy_process_group()
'''


def test_two_ranks_sharded_on_device(G, tmp_path):
    """the sharded path on the device: two processes (both on cuda:0 here -- the box has one GPU), each
    with the engine over its contiguous shard, exchanging only the reduced vectors through the
    all-reduce hook (gloo here; bench.py uses RCCL).  Must equal the single-rank reference golden."""
    import sys
    from conftest import REPO
    out = str(tmp_path / "rec")
    script = tmp_path / "w.py"
    script.write_text(WORKER % dict(repo=REPO, pack=os.path.join(GOLDEN, "m3.gpk"), out=out, iters=50))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29633", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r))) for r in range(2)]
    for p in procs:
        assert p.wait(timeout=600) == 0
    assert open(out + ".0").read() == open(out + ".1").read()
    mine = open(out + ".0").read().splitlines()
    golden = open(os.path.join(GOLDEN, "m3.rtrace")).read().splitlines()[:len(mine)]
    (tmp_path / "g").write_text("\n".join(golden) + "\n")
    compare_records(out + ".0", str(tmp_path / "g"))


def _records(G, pack, iters, path, env=None, comm_factory=None):
    old = {}
    for k, v in (env or {}).items():
        old[k] = os.environ.get(k)
        os.environ[k] = v
    try:
        pk = G.Pack.load(pack)
        lib = G.load_library(dims=(pk.n, pk.K, pk.B))
        comm = comm_factory(lib) if comm_factory else None
        s = G.Sampler(pk, lib=lib, comm=comm)
        s.set_record_file(path)
        s.initialize()
        for it in range(iters):
            s.iteration(it)
        s.dump_state(path + ".state", True)
        s.set_record_file(None)
        hs = s.host_stats()
        s.close()
        if comm:
            lib.gph_comm_destroy(comm)
        return hs
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("name", ["m3", "a7", "m4", "z0"])
def test_resident_decisions_equal_host_decisions(G, tmp_path, name):
    """the decisions above the loci taken by k_global on the device (one host synchronisation per iteration) against
    the same gg_stage code run on the host with a synchronisation per stage (GPH_HOST_DECISIONS=1): byte-identical
    records and final state, and both equal to the real reference's golden records"""
    iters = CASES[name]
    pack = os.path.join(GOLDEN, name + ".gpk")
    a, b = str(tmp_path / "res.rec"), str(tmp_path / "host.rec")
    hs_a = _records(G, pack, iters, a)
    hs_b = _records(G, pack, iters, b, env={"GPH_HOST_DECISIONS": "1"})
    assert hs_a["resident"] and not hs_b["resident"]
    assert open(a).read() == open(b).read()
    assert open(a + ".state").read() == open(b + ".state").read()
    compare_records(a, os.path.join(GOLDEN, name + ".rtrace"))
    # one synchronisation per iteration (+ the initialisation and the state dump) against one per stage
    assert hs_a["syncs"] <= iters + 8, hs_a
    assert hs_b["syncs"] > 4 * iters, hs_b


def test_native_rccl_communicator_single_rank(G, tmp_path):
    """the RCCL path of the engine with the one rank this box has: ncclCommInitRank from an id passed through the C
    ABI, the reduced row all-gathered on the engine's stream before every k_global stage, no host synchronisation
    inside an iteration -- records equal to the golden"""
    import ctypes

    def factory(lib):
        raw = (ctypes.c_uint8 * 128)()
        assert lib.gph_comm_unique_id(raw) == 0
        c = lib.gph_comm_create_rccl(bytes(raw), 0, 1, 0)
        assert c and lib.gph_comm_kind(c) == b"rccl"
        return c
    iters = 60
    out = str(tmp_path / "rccl.rec")
    hs = _records(G, os.path.join(GOLDEN, "m3.gpk"), iters, out, comm_factory=factory)
    assert hs["resident"] and hs["collectives"] >= 4 * iters and hs["syncs"] <= iters + 8, hs   # sweep + 2 tau + mixing per iteration
    golden = open(os.path.join(GOLDEN, "m3.rtrace")).read().splitlines()
    mine = open(out).read().splitlines()
    (tmp_path / "g").write_text("\n".join(golden[:len(mine)]) + "\n")
    compare_records(out, str(tmp_path / "g"))


@pytest.mark.parametrize("name,ranks", [("m3", 2), ("a7", 2), ("v8", 3), ("j1", 3)])
def test_launcher_ranks_share_the_device(tmp_path, name, ranks):
    """`G-PhoCS-hip -g N <control-file>`: the C launcher forks N ranks before any GPU call; with one GPU on the box the
    ranks share it and exchange through host shared memory (RCCL refuses two ranks on one GPU).  One chain, loci
    sharded, the real reference binary's trace file"""
    import shutil
    exe = os.path.join(REPO, "g-phocs_amd", "G-PhoCS-hip")
    for ext in (".ctl", ".seq"):
        shutil.copy(os.path.join(GOLDEN, name + ext), tmp_path)
    r = subprocess.run([exe, "-g", str(ranks), "-v", name + ".ctl"], cwd=tmp_path, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    compare_trace_files(os.path.join(GOLDEN, name + ".trace"), os.path.join(tmp_path, name + ".trace"))


@pytest.mark.parametrize("name", ["m4", "a7", "g2", "j1", "j2"])     # j1 / j2: bands with ancestral ends (band START events inside a chain)
def test_kernel_level_fixtures(G, name):
    """single calls of computeLocusDataLikelihood / considerEventMove / rubberBand(pre) on the device
    (gph_engine_unit) against the outputs of the real reference's own functions for the same chain state
    (tests/golden/*.unit, oracle/ref_harness.c `unit`): every value bit for bit"""
    import unit_fixture
    pk = G.Pack.load(os.path.join(GOLDEN, name + ".gpk"))
    lib = G.load_library(dims=(pk.n, pk.K, pk.B))
    assert unit_fixture.check_unit(G, lib, GOLDEN, name) > 100
    # second set: executeGenSPR (return codes 0 / 1 / 2), scaleAllNodeAges + revert, rubberBandRipple do / undo, traceLineage
    assert unit_fixture.check_unit2(G, lib, GOLDEN, name) > 1000


def test_native_library_is_the_path(G):
    """the ops must come from the in-tree HIP library; without it construction fails loudly"""
    import gphocs_amd
    assert os.path.exists(gphocs_amd.LIB_PATH)
    with pytest.raises(RuntimeError):
        gphocs_amd.load_library("/nonexistent/libgphocs_hip.so")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["g1", "m3", "a7", "f3", "v8", "w2", "x8", "y9", "r5", "b2", "n7", "j1", "j2", "j3",
                                  "k3",     # k3: burn-in 13: iteration numbers below zero on the device, mcmc-sample-skip 2, log period 10
                                  "p6",     # p6: 2^16 phases of one pattern (a repeated column of 16 hets), 65 554 phased patterns in one locus
                                  "p7"])    # p7: 64 phases of one pattern = the 64 phased patterns of a locus; 32 phases among 40: the lane shift of add_phases over a whole wavefront
def test_program_trace_file(name, tmp_path):
    """G-PhoCS-hip <control-file> on the MI355X: the trace file of the real G-PhoCS binary for the same
    control + sequence files (tests/golden/*.trace): parameter columns character-identical, the two log-likelihood
    columns within 1e-10 relative (GPhoCS.c:1763-1769)."""
    import shutil
    import subprocess
    exe = os.path.join(REPO, "g-phocs_amd", "G-PhoCS-hip")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    for ext in (".ctl", ".seq", ".rates"):
        if os.path.exists(os.path.join(GOLDEN, name + ext)):
            shutil.copy(os.path.join(GOLDEN, name + ext), tmp_path)
    extra = []
    if name == "w2":     # primary + secondary control file (GPhoCS.c:35-43, MCMCcontrol.c:178-210)
        shutil.copy(os.path.join(GOLDEN, "w2b.ctl"), tmp_path)
        extra = ["w2b.ctl"]
    r = subprocess.run([exe, name + ".ctl"] + extra, cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    ndiff = compare_trace_files(os.path.join(GOLDEN, name + ".trace"), os.path.join(tmp_path, name + ".trace"))
    assert ndiff <= len(open(os.path.join(GOLDEN, name + ".trace")).read().splitlines()) // 10


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["a7", "v8"])
def test_program_through_rccl_launcher(tmp_path, name):
    """tools/run_multi_gpu.py under torch.distributed.run with the nccl (= RCCL) backend and one rank on this GPU:
    the all-gather hook with device tensors, gph_run_control_file_ranked, trace file vs the real binary's"""
    import shutil
    for ext in (".ctl", ".seq"):
        shutil.copy(os.path.join(GOLDEN, name + ext), tmp_path)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", "29533", os.path.join(REPO, "tools", "run_multi_gpu.py"), name + ".ctl"]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    compare_trace_files(os.path.join(GOLDEN, name + ".trace"), os.path.join(tmp_path, name + ".trace"))


# ---------------------------------------------------------------- world > 1 on the device-resident path
def _local_comms(lib, world):
    group = lib.gph_comm_local_group(world, 0)
    assert group
    comms = [lib.gph_comm_create_local(group, r) for r in range(world)]
    assert all(comms) and lib.gph_comm_kind(comms[0]) == b"local" and lib.gph_comm_on_stream(comms[0]) == 1
    return comms


def _thread_ranks(G, pack_path, iters, world, tmp_path, comms=None, tag="rec"):
    """`world` ranks as THREADS of this process on the one GPU, each with its engine over its block of loci and a
    gph_comm_create_local() communicator: the all-gather of the reduced rows runs on the engines' streams (HIP events
    order the copies), so flush_pending's multi-rank branch -- k_reduce_stage without the fused stage, the gather into
    `world` rows, k_global combining them in rank order -- runs exactly as it does under RCCL over xGMI.
    comms: the caller's communicators (_local_comms), which stay the caller's to destroy; else a group of this run's own"""
    import threading
    pk = G.Pack.load(pack_path)
    lib = G.load_library(dims=(pk.n, pk.K, pk.B))
    own = comms is None
    if own:
        comms = _local_comms(lib, world)
    out, errs, stats = [str(tmp_path / f"{tag}.{r}") for r in range(world)], [], [None] * world

    def work(r):
        try:
            s = G.Sampler(pk, lib=lib, rank=r, world=world, comm=comms[r])
            s.set_record_file(out[r])
            s.initialize()
            for it in range(iters):
                s.iteration(it)
            s.dump_state(out[r] + ".state", True)
            s.set_record_file(None)
            stats[r] = s.host_stats()
            s.close()
        except Exception as ex:  # a failed rank must not leave the others waiting: destroying its communicator releases them
            errs.append((r, ex))
            lib.gph_comm_destroy(comms[r])
            comms[r] = None
    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=900)
    for c in comms if own else []:
        if c:
            lib.gph_comm_destroy(c)
    assert not errs, errs
    return out, stats


@pytest.mark.parametrize("name,world", [("m3", 2), ("a7", 2), ("m4", 3), ("a6", 2)])
def test_thread_ranks_run_the_resident_multi_rank_path(G, tmp_path, name, world):
    """world > 1 with the decisions on the device, on a one-GPU box: every rank writes the single-rank golden's records
    (rubber-band conflicts with the min-reduced first conflicting locus, sample-age moves, checkAll included), the
    shards' final states concatenate to the golden state, one host synchronisation per iteration"""
    iters = CASES[name]
    out, stats = _thread_ranks(G, os.path.join(GOLDEN, name + ".gpk"), iters, world, tmp_path)
    for r in range(1, world):
        assert open(out[0]).read() == open(out[r]).read()
    compare_records(out[0], os.path.join(GOLDEN, name + ".rtrace"))
    for hs in stats:
        assert hs["resident"] and hs["collectives"] >= 4 * iters and hs["syncs"] <= iters + 8, hs
    # per-locus state: the ranks' dumps, in rank order, are the golden's LOCUS blocks
    def blocks(path):
        txt = open(path).read()
        return txt[txt.index("LOCUS "):txt.rindex("ENDSTATE")]
    joined = tmp_path / "joined.state"
    gold = open(os.path.join(GOLDEN, name + ".state")).read()
    joined.write_text(gold[:gold.index("LOCUS ")] + "".join(blocks(o + ".state") for o in out) + "ENDSTATE\n")
    compare_states(str(joined), os.path.join(GOLDEN, name + ".state"), skip_global=True)


def test_thread_rank_gather_costs_one_stage_launch_and_survives_engine_reuse(G, tmp_path):
    """Thread ranks exchange their reduced rows in ONE way: reduction -> event-ordered gather on the streams -> k_global.
    Against a single rank, whose reduction kernel runs the decision stage in its own last block, that is one k_global launch
    more per reduction point with stages; the records are the single-rank golden's all the same.  And a SECOND engine on a
    communicator that has already served one (two chains one after the other on one group) writes the same records again."""
    name, iters, world = "m3", CASES["m3"], 2
    pack, gold = os.path.join(GOLDEN, name + ".gpk"), os.path.join(GOLDEN, name + ".rtrace")
    # 1. records and the resident path
    out, stats = _thread_ranks(G, pack, iters, world, tmp_path)
    assert open(out[0]).read() == open(out[1]).read()
    compare_records(out[0], gold)
    for hs in stats:
        assert hs["resident"] and hs["syncs"] <= iters + 8, hs
    assert stats[0]["collectives"] == stats[1]["collectives"], stats
    # 2. launches: the same chain on one rank (no gather, the stages fused into the reduction kernel)
    pk = G.Pack.load(pack)
    s = G.Sampler(pk, lib=G.load_library(dims=(pk.n, pk.K, pk.B)))
    s.set_record_file(str(tmp_path / "one"))
    s.initialize()
    for it in range(iters):
        s.iteration(it)
    s.set_record_file(None)
    one = s.host_stats()
    s.close()
    compare_records(str(tmp_path / "one"), gold)
    for hs in stats:
        assert hs["launches"] > one["launches"] + 3 * iters, (stats, one)
    # 3. two chains of 12 iterations, one after the other, on the same communicators
    lib = s.lib
    comms = _local_comms(lib, world)
    try:
        rounds = [_thread_ranks(G, pack, 12, world, tmp_path, comms=comms, tag=f"r{rnd}")[0] for rnd in range(2)]
    finally:
        for c in comms:
            if c:
                lib.gph_comm_destroy(c)
    recs = [[open(o).read() for o in outs] for outs in rounds]
    assert recs[0][0] == recs[0][1] and recs[1][0] == recs[1][1] and recs[0][0] == recs[1][0]
    mine = recs[1][0].splitlines()
    (tmp_path / "gp").write_text("".join(l + "\n" for l in open(gold).read().splitlines()[:len(mine)]))
    compare_records(rounds[0][0], tmp_path / "gp")
    compare_records(rounds[1][0], tmp_path / "gp")


def _ndev():
    import torch
    return torch.cuda.device_count()


@pytest.mark.parametrize("name", ["m3", "a7", "v8"])
def test_launcher_two_real_rccl_ranks(tmp_path, name):
    """`G-PhoCS-hip -g 2` with one GPU per rank: ncclCommInitRank with world 2, the stream-queued all-gather over
    xGMI between k_reduce_stage and k_global -- the real binary's trace file.  Needs a box with >= 2 GPUs."""
    if _ndev() < 2:
        pytest.skip("one GPU on this box: RCCL wants one GPU per rank (the thread-rank test covers the same engine path)")
    import shutil
    exe = os.path.join(REPO, "g-phocs_amd", "G-PhoCS-hip")
    for ext in (".ctl", ".seq"):
        shutil.copy(os.path.join(GOLDEN, name + ext), tmp_path)
    r = subprocess.run([exe, "-g", "2", "-v", name + ".ctl"], cwd=tmp_path, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "shared-memory exchange" not in r.stdout
    compare_trace_files(os.path.join(GOLDEN, name + ".trace"), os.path.join(tmp_path, name + ".trace"))


def test_bench_two_real_rccl_ranks():
    """`python bench.py --gpus 2` (no launcher around it) on a box with >= 2 GPUs: two ranks, RCCL communicator of
    world 2 as RCCL reports it, device-resident decisions, the counters of the one-rank run"""
    if _ndev() < 2:
        pytest.skip("one GPU on this box")
    import json
    args = ["--loci", "4000", "--preroll", "4", "--steps", "4", "--warmup", "1", "--no-cpu-baseline"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    lines = []
    for n in (1, 2):
        r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", str(n)] + args, capture_output=True,
                           text=True, timeout=1800, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        assert len(r.stdout.strip().splitlines()) == 1
        lines.append(json.loads(r.stdout))
    one, two = lines
    c = two["config"]
    assert two["n_gpus"] == 2 and c["loci_this_rank"] == 2000 and c["communicator"] == "rccl" and c["communicator_world"] == 2
    assert c["decisions"].startswith("device-resident") and c["host_syncs_per_iteration"] <= 1.01
    assert c["evals_timed"] == one["config"]["evals_timed"]
    assert c["accept_counts_timed"] == one["config"]["accept_counts_timed"]


@pytest.mark.parametrize("name", ["m3", "a7", "x8", "j1", "j2", "v8", "bigp", "stress", "y9@big", "b2@big", "j1@big", "a7@big"])
def test_checked_build_finds_no_index_out_of_range(G, oracle_cli, tmp_path, name):
    """round 6 ("the sanitizers in the container never see the device forms"; no GPU sanitizer on this
    pool): libgphocs_hip_chk.so is the library compiled with -DGPH_BOUNDS -- every index the DEVICE forms of the per-locus code put
    into an array of the locus's LDS image, into its dynamic LDS or into its conditional arrays is compared with the extent of
    that array; the first violation would leave its source line behind.  The goldens (migration, conflicts, sample ages, VAR
    rates, 32 leaves / 16 bands, the non-caterpillar shapes, pattern-rich loci on the generic paths) run through it with the
    golden's results and NO violation."""
    # @big: the checked build with variant b's capacities (64 leaves / 39 populations / 100 bands): the big-tree and many-band forms
    big = name.endswith("@big")
    name = name.split("@")[0]
    chk = os.path.join(REPO, "g-phocs_amd", G.CHECKED_LIB_BIG if big else G.CHECKED_LIB)
    assert os.path.exists(chk)
    lib = G.load_library(chk)
    assert lib.gph_build_id().decode().startswith("chkb-" if big else "chk-")
    pack = os.path.join(GOLDEN, name + ".gpk")
    iters = CASES.get(name, 10)
    s = G.Sampler(G.Pack.load(pack), lib=lib)
    p = str(tmp_path / "chk.rec")
    s.set_record_file(p)
    s.initialize()
    for it in range(iters):
        s.iteration(it)
    s.dump_state(p + ".state", True)
    s.set_record_file(None)
    where, checked = s.debug_oob()
    s.close()
    assert checked == 1, "not a checked build"
    assert where == 0, f"index out of range at {where} (source line + 100000 x file: 1 gph_locus.h, 2 gph_kernels.h)"
    if name in CASES:
        compare_records(p, os.path.join(GOLDEN, name + ".rtrace"))
        compare_states(p + ".state", os.path.join(GOLDEN, name + ".state"))
    else:
        ot, os_ = tmp_path / "o.trace", tmp_path / "o.state"
        subprocess.run([oracle_cli, "run", pack, str(iters), str(ot), str(os_), str(iters - 1), "1"], check=True, timeout=600)
        compare_records(p, ot)
        compare_states(p + ".state", os_)
    if name == "m3" and not big:
        # the check itself: one access one past the capacity of the node records (unit op 8) must be reported with its source line
        s = G.Sampler(G.Pack.load(pack), lib=lib)
        s.initialize()
        s.unit(8, 3)
        assert s.debug_oob() == (0, 1)
        s.unit(8, 2 * 32 - 1)
        where, _ = s.debug_oob()
        s.close()
        assert 200000 < where < 300000, where          # a line of gph_kernels.h (kb_unit)
    # a product library is not a checked build
    s2 = G.Sampler(G.Pack.load(os.path.join(GOLDEN, "g1.gpk")))
    assert s2.debug_oob() == (0, 0)
    s2.close()


@pytest.mark.parametrize("name", ["m3", "a7", "g2", "v8"])
def test_plain_build_parity(G, tmp_path, name):
    """the control build WITHOUT the backend switches the hot path is tuned with (-disable-machine-licm,
    -structurizecfg-skip-uniform-regions, max-ilp scheduling): same goldens, and byte-identical records to the tuned
    build -- a compiler whose uniformity analysis or M0 usage breaks an assumption of the tuned build shows here"""
    plain = os.path.join(REPO, "g-phocs_amd", G.PLAIN_LIB)
    assert os.path.exists(plain)
    lib = G.load_library(plain)
    assert lib.gph_build_id().decode().startswith("plain-")
    pk = G.Pack.load(os.path.join(GOLDEN, name + ".gpk"))
    recs = []
    for tag, l in (("plain", lib), ("tuned", G.load_library(dims=(pk.n, pk.K, pk.B)))):
        s = G.Sampler(pk, lib=l)
        p = str(tmp_path / f"{tag}.rec")
        s.set_record_file(p)
        s.initialize()
        for it in range(CASES[name]):
            s.iteration(it)
        s.dump_state(p + ".state", True)
        s.set_record_file(None)
        s.close()
        recs.append(p)
    compare_records(recs[0], os.path.join(GOLDEN, name + ".rtrace"))
    compare_states(recs[0] + ".state", os.path.join(GOLDEN, name + ".state"))
    assert open(recs[0]).read() == open(recs[1]).read()
    assert open(recs[0] + ".state").read() == open(recs[1] + ".state").read()


@pytest.mark.parametrize("name", ["m3", "a7", "a6", "m4"])
def test_fused_finish_equals_separate_finish_kernels(G, tmp_path, name):
    """the commit / revert of a decided UpdateTau / UpdateSampleAge proposal at the head of the next evaluate kernel
    (default) against every finish as a kernel of its own (GPH_NO_FUSE=1): byte-identical records and final state --
    rubber-band conflicts (m3), sample-age moves in both directions (a6 / a7) -- and fewer launches"""
    iters = CASES[name]
    pack = os.path.join(GOLDEN, name + ".gpk")
    a, b = str(tmp_path / "fused.rec"), str(tmp_path / "sep.rec")
    hs_a = _records(G, pack, iters, a)
    hs_b = _records(G, pack, iters, b, env={"GPH_NO_FUSE": "1"})
    assert open(a).read() == open(b).read()
    assert open(a + ".state").read() == open(b + ".state").read()
    compare_records(a, os.path.join(GOLDEN, name + ".rtrace"))
    assert hs_a["launches"] < hs_b["launches"], (hs_a, hs_b)


@pytest.mark.parametrize("name", ["m3", "g2", "x8"])
def test_root_sum_through_lds_equals_lane_reads(G, tmp_path, name):
    """the ordered per-pattern sum of the root reduction with the terms handed over through LDS (one vector instruction
    per pattern) against the lane-read form: the same additions in the same order -- byte-identical records and state"""
    pack = os.path.join(GOLDEN, name + ".gpk")
    a, b = str(tmp_path / "lds.rec"), str(tmp_path / "lane.rec")
    _records(G, pack, CASES[name], a, env={"GPH_LDS_SUM": "1"})
    _records(G, pack, CASES[name], b, env={"GPH_LDS_SUM": "0"})
    assert open(a).read() == open(b).read()
    assert open(a + ".state").read() == open(b + ".state").read()
    compare_records(a, os.path.join(GOLDEN, name + ".rtrace"))


def test_odd_leaf_count_and_pattern_rich_loci_against_live_oracle(G, oracle_cli, tmp_path):
    """13 leaves (an odd count: the last byte of a pattern's 4-bit leaf codes is half used) and loci with up to 485 phased
    patterns, 30 of the 40 with more than 64 (the side-stream launch group is the larger one here)"""
    pack = os.path.join(GOLDEN, "stress.gpk")
    tr, _, st1, _ = _run(G, pack, 10, tmp_path, "stress")
    ot, os_ = tmp_path / "o.trace", tmp_path / "o.state"
    subprocess.run([oracle_cli, "run", pack, "10", str(ot), str(os_), "9", "1"], check=True, timeout=600)
    compare_records(tr, ot)
    compare_states(st1, os_)


@pytest.mark.parametrize("budget", [5200, 6000, 8000])
def test_loci_whose_sequence_block_outgrows_lds_read_it_from_hbm(G, oracle_cli, tmp_path, budget):
    """a locus whose sequence block does not fit the LDS budget of a launch group keeps it in HBM
    (its own launch group; the reference mallocs any P, LocusDataLikelihood.c:251) instead of being refused.  GPH_HUGE_LDS
    shrinks the budget so that the `stress` pack (loci with up to 485 phased patterns at 13 leaves) runs as three launch
    groups on the MI355X: byte-identical to the run with every block in LDS, and equal to the oracle"""
    pack = os.path.join(GOLDEN, "stress.gpk")
    a, b = str(tmp_path / "lds.rec"), str(tmp_path / "hbm.rec")
    _records(G, pack, 10, a)
    _records(G, pack, 10, b, env={"GPH_HUGE_LDS": str(budget)})
    assert open(a).read() == open(b).read()
    assert open(a + ".state").read() == open(b + ".state").read()
    ot, os_ = tmp_path / "o.trace", tmp_path / "o.state"
    subprocess.run([oracle_cli, "run", pack, "10", str(ot), str(os_), "9", "1"], check=True, timeout=600)
    compare_records(b, ot)
    compare_states(b + ".state", os_)


@pytest.mark.parametrize("budget", [5200, 8000])
def test_variable_locus_rates_with_sequence_blocks_in_hbm(G, oracle_cli, tmp_path, budget):
    """round 6 (ADVICE): `locus-mut-rate VAR` with loci whose sequence block stays in HBM -- refused at the
    first UpdateLocusRate until round 5.  The `stress` pack as a VAR chain (alpha 1.4, step 0.9), blocks forced into HBM by
    GPH_HUGE_LDS: byte-identical to the run with every block in LDS, and equal to the oracle's serial loop (GPhoCS.c:4598-4680)"""
    from gphocs_amd_pkg import synth
    pk = synth.make_var_rates(G.Pack.load(os.path.join(GOLDEN, "stress.gpk")), 1.4, 0.9)
    pack = str(tmp_path / "stress_var.gpk")
    synth.write_pack(pk, pack)
    a, b = str(tmp_path / "lds.rec"), str(tmp_path / "hbm.rec")
    _records(G, pack, 12, a)
    _records(G, pack, 12, b, env={"GPH_HUGE_LDS": str(budget)})
    assert open(a).read() == open(b).read()
    assert open(a + ".state").read() == open(b + ".state").read()
    ot, os_ = tmp_path / "o.trace", tmp_path / "o.state"
    subprocess.run([oracle_cli, "run", pack, "12", str(ot), str(os_), "11", "1"], check=True, timeout=600)
    compare_records(b, ot)
    compare_states(b + ".state", os_)
    assert sum(int(l.split()[3]) for l in open(b) if " LRATE " in l) > 20


def test_side_stream_equals_serial_launch_groups(G, tmp_path):
    """the launch group of the pattern-rich loci (P > 64) runs next to the main group on a side stream, forked from and
    joined to the engine's stream per launch point; GPH_SIDE_STREAM=0 runs the two groups one after the other:
    byte-identical records and state (golden bigp: one locus with 75 patterns among 16)"""
    pack = os.path.join(GOLDEN, "bigp.gpk")
    a, b = str(tmp_path / "side.rec"), str(tmp_path / "serial.rec")
    _records(G, pack, 40, a)
    _records(G, pack, 40, b, env={"GPH_SIDE_STREAM": "0"})
    assert open(a).read() == open(b).read()
    assert open(a + ".state").read() == open(b + ".state").read()


@pytest.mark.parametrize("name", ["m3", "a7", "x8"])
def test_sequence_block_forms_agree(G, tmp_path, name):
    """the sequence block keeps pattern counts as 16-bit words when every count of the data set allows it and the root
    sum takes its LDS form per locus, where the terms fit behind the block; the 32-bit counts (GPH_CNT16=0) and the
    default group sizing (neither form forced) give byte-identical records and state, equal to the reference's"""
    pack = os.path.join(GOLDEN, name + ".gpk")
    a, b = str(tmp_path / "c16.rec"), str(tmp_path / "c32.rec")
    _records(G, pack, CASES[name], a)
    _records(G, pack, CASES[name], b, env={"GPH_CNT16": "0"})
    assert open(a).read() == open(b).read()
    assert open(a + ".state").read() == open(b + ".state").read()
    compare_records(a, os.path.join(GOLDEN, name + ".rtrace"))


def test_reinitialise_drops_an_owed_mixing_commit(G, tmp_path):
    """gph_engine_init_genealogies with a mixing commit still owed to the next sweep kernel (device-resident
    iteration: the decision is taken by k_global, the commit rides at the head of k_sweep)"""
    from parity_util import reinit_after_accepted_mixing
    pk = G.Pack.load(os.path.join(GOLDEN, "m3.gpk"))
    reinit_after_accepted_mixing(G, G.load_library(dims=(pk.n, pk.K, pk.B)), os.path.join(GOLDEN, "m3.gpk"), tmp_path)


def test_stepwise_entry_points(G, tmp_path):
    """gph_engine_genealogy_sweep against gph_mcmc_update_gb; tau evaluate + revert and mixing evaluate leave the loci as they
    were (parity_util.stepwise_entry_points), on the device library of each golden's dimensions"""
    from parity_util import stepwise_entry_points
    stepwise_entry_points(G, lambda pk: G.load_library(dims=(pk.n, pk.K, pk.B)), GOLDEN, tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("victim,second", [(11, 14), (13, 15)])
def test_fatal_error_names_the_locus_and_prints_its_genealogy(G, tmp_path, capfd, victim, second):
    """a per-locus fatal error on the MI355X names the first failing locus (it rides next to the
    code in the reduced row) and prints that locus's genealogy and event chains, as printGenealogyAndExit does upstream
    (GPhoCS.c:660-676); gph_engine_last_error returns both"""
    from test_host_logic import fatal_error_names_the_locus
    pk = G.Pack.load(os.path.join(GOLDEN, "m3.gpk"))
    lib = G.load_library(dims=(pk.n, pk.K, pk.B))
    # (13: the chain of population 1 is broken before its SAMPLES_START event -- the leaf walk of traceLineage, bounded since
    # round 5, ends with Fatal Error 0101 instead of spinning)
    locus, code = fatal_error_names_the_locus(G, lib, tmp_path, victim=victim, second=second)
    err = capfd.readouterr().err
    assert f"Fatal Error {code:04d}" in err and f"first in locus {locus}" in err
    assert f"LOCUS {locus} root" in err and "\nC 0" in err and "\nN 0 " in err
