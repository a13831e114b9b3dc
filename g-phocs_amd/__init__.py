"""g-phocs_amd: host-side Python mirror of the C ABI of libgphocs_hip.so (include/gphocs_hip.h),
the MI355X-native per-locus likelihood engine for G-PhoCS-style MCMC.

The package directory name contains a hyphen (it is fixed by the project layout), so import it
through the repo-root alias module `gphocs_amd` (gphocs_amd.py) or importlib.

Python is plumbing only: parsing packs, handing plain buffers to the C ABI, and (multi-GPU)
providing the RCCL all-reduce through torch.distributed.  All computation is in the HIP library;
if the library (or a GPU) is missing, construction fails loudly -- there is no CPU fallback.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from .synth import make_synthetic_pack, replicate_pack, write_pack  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(_HERE)
LIB_PATH = os.path.join(_HERE, "libgphocs_hip.so")
CSRC = os.path.join(_HERE, "csrc")

# -disable-machine-licm: the machine-level loop-invariant code motion hoists constants (a 64-bit 0.0, 1e-6) and
# lane-derived masks out of the proposal loops of the sweep kernel into registers it then has to spill to scratch
# memory -- and reload, hundreds of cycles each, ~10 times per proposal.  Without it the sweep kernel has no vector
# spills at 80 VGPRs (25 before) and 23 instead of 47 scalar spills: -5.4 % sweep time (profiles/HISTORY.md, round 1, v16).
# -structurizecfg-skip-uniform-regions: the backend's CFG structurizer runs on EVERY region by default, also on those
# whose branches are all wave-uniform (nearly all of this code: the chain logic branches on scalars).  Structurizing
# rewrites multi-exit loops and unstructured merges with guard flags (lane masks carried through phis) and pays for
# the extra merges with register copies in the loop bodies; leaving uniform regions as the plain scalar-branch CFG
# they are: -5 % sweep time, -7..18 % static instructions per kernel (profiles/HISTORY.md, round 2).
# -amdgpu-sched-strategy=max-ilp: the sweep kernel is issue-bound at a fixed occupancy (launch bounds), so the
# scheduler has nothing to gain from trading latency hiding for registers: -0.7 % -- for the variants built for 6
# wavefronts per SIMD (80 VGPRs, no spill).  Variant s is built for 8 (64 VGPRs): there the default scheduler spills 18
# vector registers instead of 23 and is the 0.7 % faster one (HIPCC_TUNING_SPILLING).
HIPCC_BASE = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
              "-Wno-unused-result", "-pthread"]
HIPCC_TUNING = ["-mllvm", "-disable-machine-licm", "-mllvm", "-structurizecfg-skip-uniform-regions",
                "-mllvm", "-amdgpu-sched-strategy=max-ilp"]
HIPCC_TUNING_SPILLING = HIPCC_TUNING[:4]
HIPCC_FLAGS = HIPCC_BASE + HIPCC_TUNING
HIPCC_LIBS = ["-ldl", "-lrt"]        # after the sources: an --as-needed linker drops libraries named before their users
# The tuning switches above are backend options of THIS compiler (uniformity analysis decides what
# -structurizecfg-skip-uniform-regions leaves alone): the version they were validated with is recorded, build() warns when hipcc
# differs, and a control build WITHOUT them (`libgphocs_hip_plain.so`) runs the golden parity tests next to the
# tuned one (tests/test_gpu_parity.py::test_plain_build_parity), so a compiler change that breaks an assumption
# shows as a difference between the two.
HIPCC_VALIDATED = "roc-7.2.0 26014"
PLAIN_LIB = "libgphocs_hip_plain.so"    # capacities of variant `m`, no -mllvm switches
CHECKED_LIB = "libgphocs_hip_chk.so"    # capacities of variant `x`, -DGPH_BOUNDS: every index of the device code checked (tests only)
CHECKED_LIB_BIG = "libgphocs_hip_chkb.so"   # the same with the capacities of variant `b`: the big-tree (multi-word node sets, list-driven order) and many-band forms

# Capacity variants of the same library (same C ABI, same sources): the static LDS image of a locus is
# sized by compile-time capacities (csrc/gph_types.h), and a tighter image means more resident
# wavefronts per CU.  `load_library(dims=...)` picks the smallest variant that fits the model.
VARIANTS = {  # name: (max leaves, max pops, max bands, waves per SIMD of the sweep kernel, file)
    "s": (16, 9, 4, 8, "libgphocs_hip_s.so"),     # BASELINE configs[0..3]; its image + a 64-pattern block fit 4 LDS granules: 32 loci per CU, 8 wavefronts per SIMD (64 VGPRs, spills outside the inner loops: measured faster than 7 and 6)
    "l": (20, 13, 4, 6, "libgphocs_hip_l.so"),    # BASELINE configs[4] (20 leaves, 13 populations)
    "m": (24, 16, 8, 6, "libgphocs_hip.so"),
    "x": (32, 32, 16, 6, "libgphocs_hip_x.so"),   # the largest variant with one genealogy node per lane (2n-1 <= 63) and 32-bit population sets
    # the engine's hard caps: 64 leaves, the reference's own 39 populations (NSPECIES 20), 16 bands -- 128-bit node sets,
    # 64-bit population sets, 16-bit event ids, list-driven pruning order instead of the lane-per-node wave programs
    "g": (48, 16, 8, 6, "libgphocs_hip_g.so"),    # many samples, few populations (e.g. 20 diploids over 5 populations): the big-tree forms with a 9-KB image
    "h": (64, 40, 16, 6, "libgphocs_hip_h.so"),
    # more than 16 migration bands, up to the reference's MAX_MIG_BANDS 100 (patch.h:17): the live-band list of a chain walk in LDS
    # instead of 16 nibbles of a scalar, the model read from the chain state in HBM by every kernel (it no longer fits the
    # kernel-argument segment), 384-column reduced rows; with the 64-leaf / 39-population forms of `h`: the engine's hard caps
    "b": (64, 40, 100, 6, "libgphocs_hip_b.so"),
    # the reference's own compile-time caps (NS 200, 39 populations, MAX_MIG_BANDS 100: patch.h:17-22): node sets of seven 64-bit
    # words, the scalar pad in two registers, a 44-KB LDS image (3 loci resident per CU) -- a capability build
    "n": (200, 40, 100, 2, "libgphocs_hip_n.so"),
}


LIB_SOURCES = ("gph_engine.hip", "gph_mcmc.cpp", "gph_input.cpp", "gph_program.cpp", "gph_readtrace.cpp", "gph_comm.cpp")


def variant_for(n, K, B):
    for name in ("s", "l", "m", "x", "g", "h", "b", "n"):
        cl, ck, cb, _, _ = VARIANTS[name]
        if n <= cl and K <= ck and B <= cb:
            return name
    raise RuntimeError(f"model (leaves={n}, pops={K}, bands={B}) exceeds the engine's caps (200 leaves, 39 populations, "
                       f"100 bands); the reference's own compile-time caps are "
                       f"200 leaves / 39 populations / 100 bands (upstream src/patch.h:17-22)")


def lib_path(name="m"):
    return os.path.join(_HERE, VARIANTS[name][4])


def build(verbose=False):
    """Compile the HIP engine for gfx950 in-tree (hipcc cross-compiles without a GPU), every variant.  Safe to call from
    several processes at once (one rank per GPU all call it): an exclusive file lock serialises them, the first one
    builds what is out of date into a temporary file and renames it, the others find everything up to date."""
    import fcntl
    with open(os.path.join(_HERE, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            return _build_locked(verbose)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)


def _run_to(cmd, out, verbose):
    tmp = f"{out}.tmp.{os.getpid()}"
    if verbose:
        print(" ".join(cmd + ["-o", out]))
    try:
        subprocess.run(cmd + ["-o", tmp], check=True)
        os.replace(tmp, out)
    finally:
        if os.path.exists(tmp):
            os.unlink(tmp)


def hipcc_version():
    try:
        out = subprocess.run(["hipcc", "--version"], capture_output=True, text=True, timeout=60).stdout
    except Exception:  # pragma: no cover
        return ""
    for ln in out.splitlines():
        if "clang version" in ln:
            return ln.strip()
    return out.strip().splitlines()[0] if out.strip() else ""


def _build_locked(verbose):
    ver = hipcc_version()
    if ver and HIPCC_VALIDATED not in ver:
        print(f"gphocs_amd.build: hipcc is '{ver}', the backend switches {HIPCC_TUNING[1::2]} were validated with "
              f"'{HIPCC_VALIDATED}': run the -m gpu parity suite (it compares the tuned build with the plain one)")
    srcs = [os.path.join(CSRC, f) for f in LIB_SOURCES]
    import hashlib
    hashed = sorted(set(LIB_SOURCES) | {f for f in os.listdir(CSRC) if f.endswith(".h")})

    def build_id(flags):
        """sources + flags: what the binary is a function of besides the compiler.  The compiler's version is recorded next
        to it (sidecar, bench line) and NOT hashed: a library that travelled to a box with another hipcc -- or none -- is
        still the build of these sources, and recompiling it there would put an unvalidated compiler's code (and minutes
        of build time) inside a measurement.  Only the translation units and headers count: an editor's backup file in
        csrc/ does not make the libraries stale."""
        h = hashlib.sha256()
        for f in hashed:
            h.update(f.encode() + b"\0" + open(os.path.join(CSRC, f), "rb").read())
        h.update(" ".join(flags).encode())
        return h.hexdigest()[:12]
    deps = srcs + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")] + \
        [os.path.join(REPO, "include", "gphocs_hip.h")]
    hdr = hashlib.sha256(open(deps[-1], "rb").read()).hexdigest()[:8]

    def library(out, tag, fl):
        """up to date = built from exactly these sources with these flags: the id the library was built with sits in a
        sidecar file next to it (time stamps do not survive checkouts and snapshot copies reliably, and a rebuild on the
        GPU box costs minutes of the measurement budget); the sidecar's third field is the compiler that built it"""
        want = f"{tag}-{build_id(fl)}"
        side = out + ".buildid"
        try:
            if os.path.exists(out):
                got = open(side).read().strip().split(":", 2)
                if got[:2] == [want, hdr]:
                    built_by = got[2] if len(got) > 2 else ""
                    if ver and built_by and built_by != ver and verbose:
                        print(f"gphocs_amd.build: {os.path.basename(out)} was built by '{built_by}', this box has '{ver}': kept")
                    return
        except OSError:
            pass
        if not ver:
            if os.path.exists(out):
                print(f"gphocs_amd.build: no hipcc here; using the existing {os.path.basename(out)} although its build id "
                      f"cannot be confirmed as {want}")
                return
            raise RuntimeError(f"gphocs_amd.build: hipcc not found and {out} does not exist")
        _run_to(["hipcc"] + fl + [f'-DGPH_BUILD_ID="{want}"'] + srcs + HIPCC_LIBS, out, verbose)
        with open(side, "w") as f:
            f.write(f"{want}:{hdr}:{ver}\n")

    jobs = []
    for name, (cl, ck, cb, waves, fn) in VARIANTS.items():
        jobs.append((os.path.join(_HERE, fn), name,
                     HIPCC_BASE + (HIPCC_TUNING_SPILLING if waves > 6 else HIPCC_TUNING) +
                     [f"-DGPH_CAP_LEAVES={cl}", f"-DGPH_CAP_K={ck}", f"-DGPH_CAP_B={cb}", f"-DGPH_SWEEP_WAVES={waves}"]))
    # control build without the backend switches (parity tests only)
    cl, ck, cb, waves, _ = VARIANTS["m"]
    jobs.append((os.path.join(_HERE, PLAIN_LIB), "plain",
                 HIPCC_BASE + [f"-DGPH_CAP_LEAVES={cl}", f"-DGPH_CAP_K={ck}", f"-DGPH_CAP_B={cb}", f"-DGPH_SWEEP_WAVES={waves}",
                               "-DGPH_LOGSTEPS"]))     # + the decision-level transcript (tests/test_logsteps.py)
    # checked build (tests only): every index of the per-locus device code against its array's extent (gph_rt.h: GPH_BOUNDS)
    cl, ck, cb, waves, _ = VARIANTS["x"]
    jobs.append((os.path.join(_HERE, CHECKED_LIB), "chk",
                 HIPCC_BASE + HIPCC_TUNING + [f"-DGPH_CAP_LEAVES={cl}", f"-DGPH_CAP_K={ck}", f"-DGPH_CAP_B={cb}", f"-DGPH_SWEEP_WAVES={waves}",
                                              "-DGPH_BOUNDS"]))
    cl, ck, cb, waves, _ = VARIANTS["b"]
    jobs.append((os.path.join(_HERE, CHECKED_LIB_BIG), "chkb",
                 HIPCC_BASE + HIPCC_TUNING + [f"-DGPH_CAP_LEAVES={cl}", f"-DGPH_CAP_K={ck}", f"-DGPH_CAP_B={cb}", f"-DGPH_SWEEP_WAVES={waves}",
                                              "-DGPH_BOUNDS"]))
    # every variant is one hipcc process of its own (half a minute each): a few at a time
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=max(1, min(5, (os.cpu_count() or 2) // 2))) as ex:
        for f in [ex.submit(library, *j) for j in jobs]:
            f.result()
    # the program: same command line as the reference's G-PhoCS binary (GPhoCS.c:84-238)
    exe, main = os.path.join(_HERE, "G-PhoCS-hip"), os.path.join(CSRC, "gph_main.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(main), os.path.getmtime(deps[-1])):
        _run_to(["g++", "-O2", "-std=c++17", "-I", os.path.join(REPO, "include"), main, "-ldl"], exe, verbose)
    # the post-run trace summary tool (readTrace.c), host only
    exe, main = os.path.join(_HERE, "readTrace"), os.path.join(CSRC, "gph_readtrace.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(main), os.path.getmtime(deps[-1])):
        _run_to(["g++", "-O2", "-std=c++17", "-DGPH_READTRACE_MAIN", main], exe, verbose)
    return LIB_PATH


# ------------------------------------------------------------------------------------ C types
class GphConfig(C.Structure):
    _fields_ = [("n", C.c_int32), ("Kc", C.c_int32), ("K", C.c_int32), ("B", C.c_int32),
                ("rootPop", C.c_int32),
                ("samplesPerPop", C.POINTER(C.c_int32)), ("popFather", C.POINTER(C.c_int32)),
                ("popSon0", C.POINTER(C.c_int32)), ("popSon1", C.POINTER(C.c_int32)),
                ("bandSrc", C.POINTER(C.c_int32)), ("bandTgt", C.POINTER(C.c_int32)),
                ("device", C.c_int32), ("L_total", C.c_int64), ("locus_begin", C.c_int64)]


class GphSweepResult(C.Structure):
    _fields_ = [("accepted_internal", C.c_int64), ("accepted_mignode", C.c_int64),
                ("accepted_spr", C.c_int64), ("dData_internal", C.c_double),
                ("dLog_internal", C.c_double), ("dLog_mignode", C.c_double),
                ("dData_spr", C.c_double), ("dLog_spr", C.c_double), ("total_mig_nodes", C.c_int64)]


class GphCounters(C.Structure):
    _fields_ = [("evals", C.c_int64), ("eval_nodes", C.c_int64), ("eval_bytes", C.c_double),
                ("not_enough_migs", C.c_int64)]


class GphMcmcConfig(C.Structure):
    _fields_ = [("thetaAlpha", C.POINTER(C.c_double)), ("thetaBeta", C.POINTER(C.c_double)),
                ("thetaStart", C.POINTER(C.c_double)), ("ageAlpha", C.POINTER(C.c_double)),
                ("ageBeta", C.POINTER(C.c_double)), ("ageStart", C.POINTER(C.c_double)),
                ("sampleAge", C.POINTER(C.c_double)), ("updateSampleAge", C.POINTER(C.c_int32)),
                ("mrAlpha", C.POINTER(C.c_double)),
                ("mrBeta", C.POINTER(C.c_double)),
                ("ftCoalTime", C.c_double), ("ftMigTime", C.c_double), ("ftTheta", C.c_double),
                ("ftMigRate", C.c_double), ("ftMixing", C.c_double),
                ("ftTaus", C.POINTER(C.c_double)),
                ("seed", C.c_int32), ("startMig", C.c_int32), ("doMixing", C.c_int32),
                ("samplesPerLog", C.c_int32), ("numParameters", C.c_int32),
                ("printFactors", C.POINTER(C.c_double)),
                ("mutRateMode", C.c_int32), ("varRatesAlpha", C.c_double), ("ftLocusRate", C.c_double)]


class GphControlInfo(C.Structure):
    _fields_ = [("seqFile", C.c_char_p), ("traceFile", C.c_char_p), ("rateFile", C.c_char_p),
                ("numLoci", C.c_int32), ("burnin", C.c_int32), ("numSamples", C.c_int32),
                ("sampleSkip", C.c_int32), ("logsPerLine", C.c_int32), ("mutRateMode", C.c_int32),
                ("findFinetunes", C.c_int32), ("findFinetunesNumSteps", C.c_int32),
                ("findFinetunesSamplesPerStep", C.c_int32), ("numSampleSlots", C.c_int32),
                ("varRatesAlpha", C.c_double), ("ftLocusRate", C.c_double)]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int32,
                           C.POINTER(C.c_double), C.c_int32)

class GphMc3Swap(C.Structure):   # gph_mc3_swap: one decision of a swap point
    _fields_ = [("call", C.c_int32), ("lower", C.c_int32), ("beta_lower", C.c_double), ("beta_upper", C.c_double),
                ("l_lower", C.c_double), ("l_upper", C.c_double), ("lnr", C.c_double), ("u", C.c_double),
                ("accepted", C.c_int32), ("pad", C.c_int32)]


class GphRunOptions(C.Structure):   # gph_run_options: what each field switches on is said there
    _fields_ = [("size", C.c_uint32), ("ctl", C.c_char_p), ("ctl2", C.c_char_p), ("device", C.c_int32), ("verbose", C.c_int32),
                ("comm", C.c_void_p), ("rank", C.c_int32), ("world", C.c_int32), ("allreduce", ALLREDUCE_FN), ("user", C.c_void_p),
                ("locus_summary_path", C.c_char_p), ("coal_stats_prefix", C.c_char_p), ("coal_stats_rows", C.c_int32),
                ("time_slices", C.c_int32), ("ancestry_prefix", C.c_char_p), ("ancestry_rows", C.c_int32),
                ("gene_trees_prefix", C.c_char_p), ("gene_trees_loci", C.c_char_p), ("gene_trees_rows", C.c_int32),
                ("clades_prefix", C.c_char_p), ("clades_loci", C.c_char_p), ("clades_slots", C.c_int32), ("clades_min_support", C.c_double),
                ("beta", C.c_double), ("marginal_prefix", C.c_char_p), ("marginal_steps", C.c_int32), ("marginal_burnin", C.c_int32),
                ("marginal_samples", C.c_int32), ("marginal_alpha", C.c_double),
                ("mc3_chains", C.c_int32), ("mc3_heat", C.c_double), ("mc3_swap_every", C.c_int32), ("mc3_report_prefix", C.c_char_p),
                ("replicates", C.c_int32), ("replicates_prefix", C.c_char_p), ("replicates_min_freq", C.c_double),
                ("replicates_every", C.c_int32), ("ess_prefix", C.c_char_p), ("ess_loci", C.c_char_p),
                ("predictive_prefix", C.c_char_p), ("predictive_loci", C.c_char_p), ("predictive_seed", C.c_char_p), ("predictive_rows", C.c_int32),
                ("triplets_prefix", C.c_char_p), ("triplets_pops", C.c_char_p), ("triplets_loci", C.c_char_p), ("triplets_rows", C.c_int32),
                ("mutations_prefix", C.c_char_p), ("mutations_loci", C.c_char_p), ("mutations_rows", C.c_int32),
                ("simulate_prefix", C.c_char_p), ("simulate_loci", C.c_char_p), ("simulate_seed", C.c_char_p), ("simulate_rows", C.c_int32),
                ("simulate_no_sites", C.c_int32),
                ("pair_times_prefix", C.c_char_p), ("pair_times_pops", C.c_char_p), ("pair_times_grid", C.c_char_p), ("pair_times_loci", C.c_char_p),
                ("pair_times_rows", C.c_int32),
                ("sfs_prefix", C.c_char_p), ("sfs_pairs", C.c_char_p), ("sfs_loci", C.c_char_p), ("sfs_rows", C.c_int32)]


def run_control_file(lib, ctl, ctl2=None, device=0, verbose=0, comm=None, locus_summary=None, coal_stats=None, coal_stats_rows=0, time_slices=0,
                     ancestry=None, ancestry_rows=0, gene_trees=None, gene_trees_loci=None, gene_trees_rows=0,
                     clades=None, clades_loci=None, clades_slots=0, clades_min_support=None,
                     beta=None, marginal=None, marginal_steps=0, marginal_burnin=None, marginal_samples=0, marginal_alpha=0.0,
                     mc3=0, mc3_heat=0.0, mc3_swap_every=0, mc3_report=None,
                     replicates=0, replicates_out=None, replicates_min_freq=None, replicates_every=0, ess=None, ess_loci=None,
                     predictive=None, predictive_loci=None, predictive_seed=None, predictive_rows=0,
                     triplets=None, triplets_pops=None, triplets_loci=None, triplets_rows=0,
                     mutations=None, mutations_loci=None, mutations_rows=0,
                     simulate=None, simulate_loci=None, simulate_seed=None, simulate_rows=0, simulate_no_sites=False,
                     pair_times=None, pair_times_pops=None, pair_times_grid=None, pair_times_loci=None, pair_times_rows=0,
                     sfs=None, sfs_pairs=None, sfs_loci=None, sfs_rows=0):
    """gph_run: the program of the control file with the outputs that are named (paths and prefixes as str or bytes); the status.
    beta: the whole chain on the power posterior (None: the posterior, 0: the prior); marginal: the prefix of the
    marginal-likelihood ladder behind the run, marginal_steps / _samples / _alpha 0 and marginal_burnin None: the defaults.
    mc3: the number of Metropolis-coupled chains (0: off), mc3_heat 0: 0.1, mc3_swap_every 0: every iteration, negative: never,
    mc3_report: the prefix of the report file.  replicates: the number of independent replicate chains (0: off), replicates_out:
    the prefix of PREFIX.psrf.tsv / PREFIX.asdsf.tsv / PREFIX.chain<r>.trace, replicates_min_freq None: 0.1, replicates_every
    k: an ASDSF line on stdout after every k-th sample (0: off).  ess: the prefix of PREFIX.ess.tsv / PREFIX.locus-ess.tsv,
    ess_loci: the loci of the second (a SPEC as gene_trees_loci; None: all).  predictive: the prefix of PREFIX.predictive.tsv /
    PREFIX.predictive-genome.tsv, predictive_loci a SPEC, predictive_seed None: the control file's random-seed, predictive_rows
    0: the default row buffer.  triplets: the prefix of PREFIX.triplets.tsv / PREFIX.triplets-genome.tsv, triplets_pops the triples
    as "A,B,C;D,E,F" (None: all), triplets_loci a SPEC, triplets_rows 0: the default row buffer.  mutations: the prefix of PREFIX.mutations.tsv /
    PREFIX.mutations-genome.tsv, mutations_loci a SPEC, mutations_rows 0: the default row buffer.  simulate: the prefix of
    PREFIX.simulate.tsv / PREFIX.simulate-genome.tsv, simulate_loci a SPEC, simulate_seed None: the control file's random-seed,
    simulate_rows 0: the default row buffer, simulate_no_sites: the genealogy level alone.  pair_times: the prefix of
    PREFIX.pair-times.tsv / PREFIX.pair-times-genome.tsv, pair_times_pops the pairs as "A,B;A,A" (None: all), pair_times_grid
    "LO,HI,B" (None: "1e-6,1e-2,34"), pair_times_loci a SPEC, pair_times_rows 0: the default row buffer.  sfs: the prefix of
    PREFIX.sfs.tsv / PREFIX.sfs-genome.tsv, sfs_pairs the pairs as "A,B;C,D" or "none" (None: all), sfs_loci a SPEC, sfs_rows 0: the
    default row buffer"""
    def b(x):
        return os.fsencode(x) if x is not None else None
    o = GphRunOptions(size=C.sizeof(GphRunOptions), ctl=b(ctl), ctl2=b(ctl2), device=device, verbose=verbose, comm=comm,
                      locus_summary_path=b(locus_summary), coal_stats_prefix=b(coal_stats), coal_stats_rows=coal_stats_rows,
                      time_slices=time_slices, ancestry_prefix=b(ancestry), ancestry_rows=ancestry_rows,
                      gene_trees_prefix=b(gene_trees), gene_trees_loci=b(gene_trees_loci), gene_trees_rows=gene_trees_rows,
                      clades_prefix=b(clades), clades_loci=b(clades_loci), clades_slots=clades_slots,
                      clades_min_support=0.0 if clades_min_support is None else -1.0 if clades_min_support == 0 else clades_min_support,
                      beta=0.0 if beta is None else -1.0 if beta == 0 else beta,
                      marginal_prefix=b(marginal), marginal_steps=marginal_steps,
                      marginal_burnin=0 if marginal_burnin is None else -1 if marginal_burnin == 0 else marginal_burnin,
                      marginal_samples=marginal_samples, marginal_alpha=marginal_alpha,
                      mc3_chains=mc3, mc3_heat=mc3_heat, mc3_swap_every=mc3_swap_every, mc3_report_prefix=b(mc3_report),
                      replicates=replicates, replicates_prefix=b(replicates_out),
                      replicates_min_freq=0.0 if replicates_min_freq is None else -1.0 if replicates_min_freq == 0 else replicates_min_freq,
                      replicates_every=replicates_every, ess_prefix=b(ess), ess_loci=b(ess_loci),
                      predictive_prefix=b(predictive), predictive_loci=b(predictive_loci),
                      predictive_seed=None if predictive_seed is None else str(predictive_seed).encode(), predictive_rows=predictive_rows,
                      triplets_prefix=b(triplets), triplets_pops=b(triplets_pops), triplets_loci=b(triplets_loci), triplets_rows=triplets_rows,
                      mutations_prefix=b(mutations), mutations_loci=b(mutations_loci), mutations_rows=mutations_rows,
                      simulate_prefix=b(simulate), simulate_loci=b(simulate_loci),
                      simulate_seed=None if simulate_seed is None else str(simulate_seed).encode(), simulate_rows=simulate_rows,
                      simulate_no_sites=int(bool(simulate_no_sites)),
                      pair_times_prefix=b(pair_times), pair_times_pops=b(pair_times_pops), pair_times_grid=b(pair_times_grid),
                      pair_times_loci=b(pair_times_loci), pair_times_rows=pair_times_rows,
                      sfs_prefix=b(sfs), sfs_pairs=b(sfs_pairs), sfs_loci=b(sfs_loci), sfs_rows=sfs_rows)
    return lib.gph_run(C.byref(o))


EXPORTS = [  # every symbol include/gphocs_hip.h declares
    "gph_engine_create", "gph_engine_destroy", "gph_engine_set_allreduce", "gph_engine_load_loci",
    "gph_engine_set_model", "gph_engine_seed", "gph_engine_init_genealogies",
    "gph_engine_genealogy_sweep", "gph_engine_tau_evaluate", "gph_engine_tau_commit",
    "gph_engine_tau_revert", "gph_engine_mixing_evaluate", "gph_engine_mixing_commit",
    "gph_engine_mixing_revert", "gph_engine_apply_theta", "gph_engine_apply_migrate",
    "gph_engine_get_totals", "gph_engine_synchronize", "gph_engine_check_all",
    "gph_engine_get_counters", "gph_engine_dump_loci", "gph_engine_last_kernel_ms",
    "gph_engine_num_loci", "gph_engine_hbm_bytes", "gph_debug_math", "gph_engine_class_stats",
    "gph_mcmc_create", "gph_mcmc_destroy", "gph_mcmc_initialize", "gph_mcmc_set_record_file",
    "gph_mcmc_iteration", "gph_mcmc_get_state", "gph_mcmc_dump_state", "gph_mcmc_accept_counts",
    "gph_mcmc_param_vals", "gph_mcmc_tau_accept_counts", "gph_mcmc_set_finetunes", "gph_mcmc_set_log_period", "gph_engine_last_error", "gph_engine_debug_break_chain", "gph_engine_debug_oob", "gph_control_read", "gph_control_free", "gph_control_get", "gph_control_pop_name",
    "gph_control_sample_name", "gph_loci_read", "gph_loci_free", "gph_loci_arrays", "gph_run_control_file", "gph_run_control_file_ranked",
    "gph_read_trace", "gph_engine_locus_rate_update", "gph_engine_set_locus_rates", "gph_mcmc_set_locus_rate_finetune",
    "gph_mcmc_locus_rate_state", "gph_engine_set_comm", "gph_engine_host_stats", "gph_engine_set_timing",
    "gph_comm_unique_id", "gph_comm_create_rccl", "gph_comm_create_shm", "gph_comm_attach_shm", "gph_comm_shm_bytes",
    "gph_comm_destroy", "gph_comm_world", "gph_comm_rank", "gph_comm_on_stream", "gph_comm_kind",
    "gph_comm_allgather_stream", "gph_comm_allreduce_host", "gph_run_control_file_comm", "gph_device_count",
    "gph_engine_unit", "gph_build_id", "gph_build_compiler", "gph_runtime_version", "gph_engine_steplog_enable", "gph_engine_steplog_fetch", "gph_comm_local_group", "gph_comm_create_local",
    "gph_mcmc_get_chain", "gph_mcmc_set_chain", "gph_mcmc_update_gb", "gph_mcmc_update_locus_rate", "gph_mcmc_update_theta",
    "gph_mcmc_update_mig_rates", "gph_mcmc_update_tau", "gph_mcmc_update_sample_age", "gph_mcmc_mixing",
    "gph_mcmc_synchronize_events", "gph_mcmc_check_all", "gph_mcmc_initialize_genealogies",
    "gph_engine_locus_summary_enable", "gph_engine_locus_summary_sample", "gph_engine_locus_summary_columns",
    "gph_engine_locus_summary_fetch", "gph_engine_locus_summary_column_name", "gph_loci_name",
    "gph_engine_coal_stats_enable", "gph_engine_coal_stats_sample", "gph_engine_coal_stats_shape", "gph_engine_coal_stats_fetch",
    "gph_engine_coal_stats_column_name", "gph_coal_stats_write", "gph_coal_stats_discard",
    "gph_engine_coal_stats_set_chunk", "gph_coal_stats_combined",
    "gph_engine_time_slices_enable", "gph_engine_time_slices_sample", "gph_engine_time_slices_shape", "gph_engine_time_slices_fetch",
    "gph_engine_time_slices_column_name", "gph_engine_time_slices_set_chunk", "gph_time_slices_write",
    "gph_time_slices_combined", "gph_time_slices_discard",
    "gph_engine_ancestry_enable", "gph_engine_ancestry_sample", "gph_engine_ancestry_shape", "gph_engine_ancestry_fetch_loci",
    "gph_engine_ancestry_fetch_rows", "gph_engine_ancestry_column_name", "gph_ancestry_write",
    "gph_ancestry_discard",
    "gph_engine_gene_trees_enable", "gph_engine_gene_trees_sample", "gph_engine_gene_trees_shape", "gph_engine_gene_trees_selected",
    "gph_engine_gene_trees_fetch", "gph_gene_trees_write", "gph_gene_trees_discard", "gph_gene_trees_decode",
    "gph_gene_tree_newick", "gph_run", "gph_run_finish",
    "gph_engine_clades_enable", "gph_engine_clades_sample", "gph_engine_clades_shape", "gph_engine_clades_selected",
    "gph_engine_clades_fetch", "gph_clades_consensus", "gph_clades_write", "gph_clades_discard",
    "gph_engine_set_beta", "gph_engine_get_beta", "gph_mcmc_set_beta", "gph_mcmc_get_beta",
    "gph_engine_exchange_state", "gph_mcmc_exchange_state", "gph_mc3_create", "gph_mc3_destroy", "gph_mc3_iteration",
    "gph_mc3_swap_counts", "gph_mc3_swap_log", "gph_engine_clades_compare", "gph_psrf",
    "gph_ess", "gph_ess_read", "gph_engine_ess_enable", "gph_engine_ess_sample", "gph_engine_ess_shape", "gph_engine_ess_selected",
    "gph_engine_ess_fetch", "gph_ess_write", "gph_ess_discard", "gph_read_trace_ess", "gph_engine_last_error_text",
    "gph_engine_predictive_enable", "gph_engine_predictive_sample", "gph_engine_predictive_shape", "gph_engine_predictive_selected",
    "gph_engine_predictive_fetch_loci", "gph_engine_predictive_fetch_rows", "gph_engine_predictive_column_name",
    "gph_predictive_write", "gph_predictive_discard",
    "gph_engine_triplets_enable", "gph_engine_triplets_sample", "gph_engine_triplets_shape", "gph_engine_triplets_selected",
    "gph_engine_triplets_fetch_loci", "gph_engine_triplets_fetch_rows", "gph_engine_triplets_column_name",
    "gph_triplets_write", "gph_triplets_discard",
    "gph_engine_mutations_enable", "gph_engine_mutations_sample", "gph_engine_mutations_shape", "gph_engine_mutations_selected",
    "gph_engine_mutations_fetch_loci", "gph_engine_mutations_fetch_rows", "gph_engine_mutations_column_name",
    "gph_mutations_write", "gph_mutations_discard",
    "gph_engine_simulate_enable", "gph_engine_simulate_sample", "gph_engine_simulate_shape", "gph_engine_simulate_selected",
    "gph_engine_simulate_fetch_loci", "gph_engine_simulate_fetch_rows", "gph_engine_simulate_fetch_records", "gph_engine_simulate_column_name",
    "gph_simulate_write", "gph_simulate_discard",
    "gph_engine_pair_times_enable", "gph_engine_pair_times_sample", "gph_engine_pair_times_shape", "gph_engine_pair_times_selected",
    "gph_engine_pair_times_fetch_loci", "gph_engine_pair_times_fetch_rows", "gph_engine_pair_times_column_name",
    "gph_pair_times_write", "gph_pair_times_discard",
    "gph_engine_sfs_enable", "gph_engine_sfs_sample", "gph_engine_sfs_shape", "gph_engine_sfs_selected", "gph_engine_sfs_slots",
    "gph_engine_sfs_fetch_loci", "gph_engine_sfs_fetch_observed", "gph_engine_sfs_fetch_rows", "gph_engine_sfs_column_name",
    "gph_sfs_write", "gph_sfs_discard",
]


_LIBS = {}


def load_library(path=None, dims=None):
    """dims = (leaves, pops, bands): load the tightest capacity variant that fits"""
    if path is None and dims is not None:
        path = lib_path(variant_for(*dims))
    path = path or LIB_PATH
    if path in _LIBS:
        return _LIBS[path]
    lib = _load_library(path)
    _LIBS[path] = lib
    return lib


def _load_library(path):
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = C.CDLL(path)
    for name in EXPORTS:
        getattr(lib, name)  # AttributeError if an ABI symbol is missing
    lib.gph_engine_num_loci.restype = C.c_int64
    lib.gph_engine_destroy.restype = None
    lib.gph_mcmc_destroy.restype = None
    lib.gph_engine_seed.argtypes = [C.c_void_p, C.c_uint32]
    lib.gph_engine_tau_revert.argtypes = [C.c_void_p, C.c_int64]
    lib.gph_engine_mixing_evaluate.argtypes = [C.c_void_p, C.c_double, C.POINTER(C.c_double)]
    lib.gph_engine_mixing_commit.argtypes = [C.c_void_p, C.c_double, C.c_double]
    lib.gph_engine_genealogy_sweep.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_double,
                                               C.POINTER(GphSweepResult)]
    lib.gph_engine_apply_theta.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_double]
    lib.gph_engine_apply_migrate.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_double]
    lib.gph_engine_load_loci.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]
    lib.gph_mcmc_iteration.argtypes = [C.c_void_p, C.c_int32]
    lib.gph_mcmc_dump_state.argtypes = [C.c_void_p, C.c_char_p, C.c_int32]
    lib.gph_engine_dump_loci.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.c_int32]
    lib.gph_engine_last_error.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    lib.gph_engine_last_error_text.argtypes = [C.c_void_p]
    lib.gph_engine_last_error_text.restype = C.c_char_p
    lib.gph_engine_debug_break_chain.argtypes = [C.c_void_p, C.c_int64, C.c_int32]
    lib.gph_mcmc_set_record_file.argtypes = [C.c_void_p, C.c_char_p]
    lib.gph_engine_last_kernel_ms.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_double)]
    lib.gph_engine_get_counters.argtypes = [C.c_void_p, C.POINTER(GphCounters), C.c_int32]
    lib.gph_engine_set_allreduce.argtypes = [C.c_void_p, ALLREDUCE_FN, C.c_void_p]
    lib.gph_mcmc_param_vals.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    lib.gph_mcmc_tau_accept_counts.argtypes = [C.c_void_p, C.c_void_p]
    lib.gph_mcmc_set_finetunes.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double,
                                           C.c_void_p]
    lib.gph_control_read.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p)]
    lib.gph_control_free.argtypes = [C.c_void_p]
    lib.gph_control_free.restype = None
    lib.gph_control_get.argtypes = [C.c_void_p, C.POINTER(GphConfig), C.POINTER(GphMcmcConfig),
                                    C.POINTER(GphControlInfo)]
    lib.gph_control_pop_name.argtypes = [C.c_void_p, C.c_int32]
    lib.gph_control_pop_name.restype = C.c_char_p
    lib.gph_control_sample_name.argtypes = [C.c_void_p, C.c_int32]
    lib.gph_control_sample_name.restype = C.c_char_p
    lib.gph_loci_read.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.POINTER(C.c_void_p), C.c_char_p, C.c_int32]
    lib.gph_loci_free.argtypes = [C.c_void_p]
    lib.gph_loci_free.restype = None
    lib.gph_loci_arrays.argtypes = [C.c_void_p] + [C.c_void_p] * 8
    lib.gph_run_control_file.argtypes = [C.c_char_p, C.c_char_p, C.c_int32, C.c_int32]
    lib.gph_run_control_file_ranked.argtypes = [C.c_char_p, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                ALLREDUCE_FN, C.c_void_p]
    lib.gph_comm_unique_id.argtypes = [C.c_void_p]
    lib.gph_comm_create_rccl.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
    lib.gph_comm_create_rccl.restype = C.c_void_p
    lib.gph_comm_create_shm.argtypes = [C.c_char_p, C.c_int32, C.c_int32]
    lib.gph_comm_create_shm.restype = C.c_void_p
    lib.gph_comm_destroy.argtypes = [C.c_void_p]
    lib.gph_comm_destroy.restype = None
    lib.gph_comm_kind.argtypes = [C.c_void_p]
    lib.gph_comm_kind.restype = C.c_char_p
    lib.gph_engine_set_comm.argtypes = [C.c_void_p, C.c_void_p]
    lib.gph_engine_host_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                          C.POINTER(C.c_int32)]
    lib.gph_engine_set_timing.argtypes = [C.c_void_p, C.c_uint32]
    lib.gph_engine_unit.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.c_int32]
    lib.gph_run_control_file_comm.argtypes = [C.c_char_p, C.c_char_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.gph_build_id.restype = C.c_char_p
    lib.gph_build_compiler.restype = C.c_char_p
    lib.gph_engine_steplog_enable.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_int32, C.c_int32]
    lib.gph_engine_steplog_fetch.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_int32), C.c_int32]
    lib.gph_runtime_version.restype = C.c_char_p
    lib.gph_comm_local_group.argtypes = [C.c_int32, C.c_int32]
    lib.gph_comm_local_group.restype = C.c_void_p
    lib.gph_comm_create_local.argtypes = [C.c_void_p, C.c_int32]
    lib.gph_comm_create_local.restype = C.c_void_p
    lib.gph_comm_world.argtypes = [C.c_void_p]
    lib.gph_comm_rank.argtypes = [C.c_void_p]
    lib.gph_comm_on_stream.argtypes = [C.c_void_p]
    lib.gph_comm_attach_shm.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.gph_comm_attach_shm.restype = C.c_void_p
    lib.gph_engine_locus_summary_enable.argtypes = [C.c_void_p, C.c_int32]
    lib.gph_engine_locus_summary_sample.argtypes = [C.c_void_p]
    lib.gph_engine_locus_summary_columns.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    lib.gph_engine_locus_summary_fetch.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int64, C.c_int32]
    lib.gph_engine_locus_summary_column_name.argtypes = [C.c_void_p, C.c_int32]
    lib.gph_engine_locus_summary_column_name.restype = C.c_char_p
    lib.gph_loci_name.argtypes = [C.c_void_p, C.c_int64]
    lib.gph_loci_name.restype = C.c_char_p
    lib.gph_engine_coal_stats_enable.argtypes = [C.c_void_p, C.c_int32]
    lib.gph_engine_coal_stats_sample.argtypes = [C.c_void_p, C.c_int32]
    lib.gph_engine_coal_stats_shape.argtypes = [C.c_void_p] + [C.POINTER(C.c_int32)] * 4
    lib.gph_engine_coal_stats_fetch.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_int32)]
    lib.gph_engine_coal_stats_column_name.argtypes = [C.c_void_p, C.c_int32]
    lib.gph_engine_coal_stats_column_name.restype = C.c_char_p
    lib.gph_coal_stats_write.argtypes = [C.c_char_p, C.c_int32]
    lib.gph_coal_stats_discard.argtypes = [C.c_char_p, C.c_int32]
    lib.gph_engine_coal_stats_set_chunk.argtypes = [C.c_void_p, C.c_int32]
    lib.gph_coal_stats_combined.argtypes = [C.c_char_p, C.c_int32, C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    lib.gph_engine_time_slices_enable.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.gph_engine_time_slices_sample.argtypes = [C.c_void_p, C.c_int32]
    lib.gph_engine_time_slices_shape.argtypes = [C.c_void_p] + [C.POINTER(C.c_int32)] * 6
    lib.gph_engine_time_slices_fetch.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_int32)]
    lib.gph_engine_time_slices_column_name.argtypes = [C.c_void_p, C.c_int32]
    lib.gph_engine_time_slices_column_name.restype = C.c_char_p
    lib.gph_engine_time_slices_set_chunk.argtypes = [C.c_void_p, C.c_int32]
    lib.gph_time_slices_write.argtypes = [C.c_char_p, C.c_int32]
    lib.gph_time_slices_discard.argtypes = [C.c_char_p, C.c_int32]
    lib.gph_time_slices_combined.argtypes = [C.c_char_p, C.c_int32, C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    lib.gph_engine_ancestry_enable.argtypes = [C.c_void_p, C.c_int32, C.c_int64]
    lib.gph_engine_ancestry_sample.argtypes = [C.c_void_p, C.c_int32]
    lib.gph_engine_ancestry_shape.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    lib.gph_engine_ancestry_fetch_loci.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int64, C.c_int32]
    lib.gph_engine_ancestry_fetch_rows.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int64, C.c_int32, C.POINTER(C.c_int32)]
    lib.gph_engine_ancestry_column_name.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.gph_engine_ancestry_column_name.restype = C.c_char_p
    lib.gph_ancestry_write.argtypes = [C.c_char_p, C.c_int32]
    lib.gph_ancestry_discard.argtypes = [C.c_char_p, C.c_int32]
    lib.gph_engine_gene_trees_enable.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.c_int64, C.c_int64]
    lib.gph_engine_gene_trees_sample.argtypes = [C.c_void_p, C.c_int32]
    lib.gph_engine_gene_trees_shape.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                                C.POINTER(C.c_int32)]
    lib.gph_engine_gene_trees_selected.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_int64)]
    lib.gph_engine_gene_trees_fetch.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
    lib.gph_gene_trees_write.argtypes = [C.c_char_p, C.c_int32]
    lib.gph_gene_trees_discard.argtypes = [C.c_char_p, C.c_int32]
    lib.gph_gene_trees_decode.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_int32), C.c_int32] + [C.c_void_p] * 14
    lib.gph_run.argtypes = [C.POINTER(GphRunOptions)]
    lib.gph_run_finish.argtypes = [C.POINTER(GphRunOptions), C.c_int32, C.c_int32]
    lib.gph_gene_tree_newick.argtypes = [C.c_int32] + [C.c_void_p] * 5 + [C.c_int32, C.c_int32] + [C.c_void_p] * 3 + \
        [C.POINTER(C.c_char_p), C.c_int32, C.POINTER(C.c_char_p), C.c_int32, C.POINTER(C.c_char_p), C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.gph_engine_clades_enable.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.c_int64, C.c_int64]
    lib.gph_engine_clades_sample.argtypes = [C.c_void_p]
    lib.gph_engine_clades_shape.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                            C.POINTER(C.c_int64)]
    lib.gph_engine_clades_selected.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_int64)]
    lib.gph_engine_clades_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    lib.gph_clades_write.argtypes = [C.c_char_p, C.c_int32]
    lib.gph_clades_discard.argtypes = [C.c_char_p, C.c_int32]
    lib.gph_mcmc_set_beta.argtypes = [C.c_void_p, C.c_double]
    lib.gph_mcmc_get_beta.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    lib.gph_engine_set_beta.argtypes = [C.c_void_p, C.c_double]
    lib.gph_engine_get_beta.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    lib.gph_engine_exchange_state.argtypes = [C.c_void_p, C.c_void_p]
    lib.gph_mcmc_exchange_state.argtypes = [C.c_void_p, C.c_void_p]
    lib.gph_mc3_create.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(C.c_double), C.c_int32, C.c_uint32, C.POINTER(C.c_void_p)]
    lib.gph_mc3_destroy.argtypes = [C.c_void_p]
    lib.gph_mc3_destroy.restype = None
    lib.gph_mc3_iteration.argtypes = [C.c_void_p, C.c_int32]
    lib.gph_mc3_swap_counts.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.gph_mc3_swap_log.argtypes = [C.c_void_p, C.POINTER(GphMc3Swap), C.c_int64, C.POINTER(C.c_int64)]
    lib.gph_engine_clades_compare.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.c_double, C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_int64)]
    lib.gph_psrf.argtypes = [C.POINTER(C.c_double), C.c_int32, C.c_int64, C.POINTER(C.c_double)]
    lib.gph_clades_consensus.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_char_p), C.c_char_p, C.c_size_t,
                                         C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]
    lib.gph_read_trace_ess.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_char_p, C.c_size_t]
    lib.gph_ess_write.argtypes = [C.c_char_p, C.c_int32]
    lib.gph_ess_discard.argtypes = [C.c_char_p, C.c_int32]
    lib.gph_ess.argtypes = [C.POINTER(C.c_double), C.c_int64, C.c_int32, C.POINTER(C.c_double)]
    lib.gph_ess_read.argtypes = [C.POINTER(C.c_double), C.c_int64, C.c_int32, C.POINTER(C.c_double)]
    lib.gph_engine_ess_enable.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_int64, C.c_int64]
    lib.gph_engine_ess_sample.argtypes = [C.c_void_p]
    lib.gph_engine_ess_shape.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                         C.POINTER(C.c_int64)]
    lib.gph_engine_ess_selected.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_int64)]
    lib.gph_engine_ess_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    lib.gph_engine_predictive_enable.argtypes = [C.c_void_p, C.c_uint64, C.c_int32, C.POINTER(C.c_int64), C.c_int64, C.c_int64]
    lib.gph_engine_predictive_sample.argtypes = [C.c_void_p, C.c_int32]
    lib.gph_engine_predictive_shape.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    lib.gph_engine_predictive_selected.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_int64)]
    lib.gph_engine_predictive_fetch_loci.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    lib.gph_engine_predictive_fetch_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
    lib.gph_engine_predictive_column_name.argtypes = [C.c_void_p, C.c_int32]
    lib.gph_engine_predictive_column_name.restype = C.c_char_p
    lib.gph_predictive_write.argtypes = [C.c_char_p, C.c_int32]
    lib.gph_predictive_discard.argtypes = [C.c_char_p, C.c_int32]
    lib.gph_engine_triplets_enable.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_int32), C.c_int32, C.c_int64]
    lib.gph_engine_triplets_sample.argtypes = [C.c_void_p, C.c_int32]
    lib.gph_engine_triplets_shape.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                              C.POINTER(C.c_int32)]
    lib.gph_engine_triplets_selected.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_int64)]
    lib.gph_engine_triplets_fetch_loci.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]
    lib.gph_engine_triplets_fetch_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_int32)]
    lib.gph_engine_triplets_column_name.argtypes = [C.c_void_p, C.c_int32]
    lib.gph_engine_triplets_column_name.restype = C.c_char_p
    lib.gph_triplets_write.argtypes = [C.c_char_p, C.c_int32]
    lib.gph_engine_pair_times_enable.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_int32), C.c_int32,
                                                 C.POINTER(C.c_double), C.c_int32, C.c_int64]
    lib.gph_engine_pair_times_sample.argtypes = [C.c_void_p, C.c_int32]
    lib.gph_engine_pair_times_shape.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64),
                                                C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_void_p]
    lib.gph_engine_pair_times_selected.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_int64)]
    lib.gph_engine_pair_times_fetch_loci.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]
    lib.gph_engine_pair_times_fetch_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_int32)]
    lib.gph_engine_pair_times_column_name.argtypes = [C.c_void_p, C.c_int32]
    lib.gph_engine_pair_times_column_name.restype = C.c_char_p
    lib.gph_pair_times_write.argtypes = [C.c_char_p, C.c_int32]
    lib.gph_pair_times_discard.argtypes = [C.c_char_p, C.c_int32]
    lib.gph_engine_sfs_enable.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_int32), C.c_int32, C.c_int64]
    lib.gph_engine_sfs_sample.argtypes = [C.c_void_p, C.c_int32]
    lib.gph_engine_sfs_shape.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64),
                                         C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    lib.gph_engine_sfs_selected.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_int64)]
    lib.gph_engine_sfs_slots.argtypes = [C.c_void_p, C.c_void_p]
    lib.gph_engine_sfs_fetch_loci.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]
    lib.gph_engine_sfs_fetch_observed.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.gph_engine_sfs_fetch_rows.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_int32)]
    lib.gph_engine_sfs_column_name.argtypes = [C.c_void_p, C.c_int32]
    lib.gph_engine_sfs_column_name.restype = C.c_char_p
    lib.gph_sfs_write.argtypes = [C.c_char_p, C.c_int32]
    lib.gph_sfs_discard.argtypes = [C.c_char_p, C.c_int32]
    lib.gph_mutations_write.argtypes = [C.c_char_p, C.c_int32]
    lib.gph_mutations_discard.argtypes = [C.c_char_p, C.c_int32]
    lib.gph_engine_mutations_enable.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.c_int64, C.c_int64]
    lib.gph_engine_mutations_sample.argtypes = [C.c_void_p, C.c_int32]
    lib.gph_engine_mutations_shape.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                               C.POINTER(C.c_int32)]
    lib.gph_engine_mutations_selected.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_int64)]
    lib.gph_engine_mutations_fetch_loci.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]
    lib.gph_engine_mutations_fetch_rows.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_int32)]
    lib.gph_engine_mutations_column_name.argtypes = [C.c_void_p, C.c_int32]
    lib.gph_engine_mutations_column_name.restype = C.c_char_p
    lib.gph_triplets_discard.argtypes = [C.c_char_p, C.c_int32]
    lib.gph_simulate_write.argtypes = [C.c_char_p, C.c_int32]
    lib.gph_simulate_discard.argtypes = [C.c_char_p, C.c_int32]
    lib.gph_engine_simulate_enable.argtypes = [C.c_void_p, C.c_uint64, C.c_int32, C.POINTER(C.c_int64), C.c_int64, C.c_int32, C.c_int64]
    lib.gph_engine_simulate_sample.argtypes = [C.c_void_p, C.c_int32]
    lib.gph_engine_simulate_shape.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                              C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    lib.gph_engine_simulate_selected.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_int64)]
    lib.gph_engine_simulate_fetch_loci.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    lib.gph_engine_simulate_fetch_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
    lib.gph_engine_simulate_fetch_records.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.gph_engine_simulate_column_name.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.gph_engine_simulate_column_name.restype = C.c_char_p
    # tests only, not in include/gphocs_hip.h (the trailing underscore): the cross-locus reduction on its own (csrc/gph_engine.hip)
    lib.gph_debug_reduce_.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                      C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_int32]
    return lib


# ------------------------------------------------------------------------------------ packs
def encode_phases(counts):
    """phase counts as the C ABI carries them (include/gphocs_hip.h: GPH_NUMPHASES): below 2^15 as they are, a power of two from
    2^15 on as 0x8000 | exponent"""
    a = np.asarray(counts, dtype=np.int64)
    big = a >= 0x8000
    if big.any():
        ex = np.round(np.log2(np.where(big, a, 1))).astype(np.int64)
        assert np.all((1 << ex[big]) == a[big]), "a phase count of 2^15 or more must be a power of two"
        a = np.where(big, 0x8000 | ex, a)
    return a.astype(np.uint16)


def decode_phases(words):
    w = np.asarray(words, dtype=np.int64)
    return np.where(w < 0x8000, w, np.left_shift(1, w & 31))


class Pack:
    """Model + processed loci (the input of gph_engine_load_loci): what the reference holds
    after readControlFile + processAlignments (GPhoCS.c:147-235).  Text format written by
    oracle/ref_harness.c `pack`; synthetic packs for the benchmark come from make_synthetic()."""

    CODES = {"T": 0, "C": 1, "A": 2, "G": 3, "N": 4}

    def __init__(self):
        self.L = 0

    @staticmethod
    def load(path):
        p = Pack()
        with open(path) as f:
            tok = f.read().split()
        it = iter(tok)

        def nxt():
            return next(it)

        def fl():
            return float.fromhex(nxt())
        assert nxt() == "GPHOCS-PACK" and nxt() == "1"
        for key in ("numLoci", "numSamples", "numCurPops", "numPops", "numMigBands", "rootPop"):
            assert nxt() == key
            setattr(p, key, int(nxt()))
        p.L, p.n, p.Kc, p.K, p.B = p.numLoci, p.numSamples, p.numCurPops, p.numPops, p.numMigBands
        assert nxt() == "samplesPerPop"
        p.samplesPerPop = np.array([int(nxt()) for _ in range(p.Kc)], dtype=np.int32)
        K, B = p.K, p.B
        p.popName = []
        p.popFather = np.zeros(K, np.int32)
        p.popSon0 = np.zeros(K, np.int32)
        p.popSon1 = np.zeros(K, np.int32)
        p.sampleAge = np.zeros(K)
        p.updateSampleAge = np.zeros(K, np.int32)
        p.thetaAlpha, p.thetaBeta, p.thetaStart = np.zeros(K), np.zeros(K), np.zeros(K)
        p.ageAlpha, p.ageBeta, p.ageStart = np.zeros(K), np.zeros(K), np.zeros(K)
        for k in range(K):
            assert nxt() == "pop" and int(nxt()) == k
            p.popName.append(nxt())
            p.popFather[k], p.popSon0[k], p.popSon1[k] = int(nxt()), int(nxt()), int(nxt())
            p.sampleAge[k] = fl()
            p.updateSampleAge[k] = int(nxt())
            p.thetaAlpha[k], p.thetaBeta[k], p.thetaStart[k] = fl(), fl(), fl()
            p.ageAlpha[k], p.ageBeta[k], p.ageStart[k] = fl(), fl(), fl()
        p.bandSrc, p.bandTgt = np.zeros(max(B, 1), np.int32), np.zeros(max(B, 1), np.int32)
        p.mrAlpha, p.mrBeta = np.zeros(max(B, 1)), np.ones(max(B, 1))
        for b in range(B):
            assert nxt() == "band" and int(nxt()) == b
            p.bandSrc[b], p.bandTgt[b] = int(nxt()), int(nxt())
            p.mrAlpha[b], p.mrBeta[b] = fl(), fl()
        assert nxt() == "mcmc"
        (p.seed, p.burnin, p.numSamplesMcmc, p.sampleSkip, p.startMig, p.doMixing, p.samplesPerLog,
         p.mutRateMode) = [int(nxt()) for _ in range(8)]
        assert nxt() == "finetunes"
        p.ftCoalTime, p.ftMigTime, p.ftTheta, p.ftMigRate, p.ftMixing = fl(), fl(), fl(), fl(), fl()
        p.ftTaus = np.array([fl() for _ in range(K)])
        key = nxt()
        p.varRatesAlpha, p.ftLocusRate = 1.0, -1.0
        if key == "locusrate":            # packs of `locus-mut-rate VAR` control files only
            p.varRatesAlpha, p.ftLocusRate = fl(), fl()
            key = nxt()
        assert key == "printFactors"
        p.numParameters = int(nxt())
        p.printFactors = np.array([fl() for _ in range(p.numParameters)])
        offs, leaf, phases, counts, rates = [0], [], [], [], []
        for g in range(p.L):
            assert nxt() == "locus" and int(nxt()) == g
            P = int(nxt())
            rates.append(fl())
            for _ in range(P):
                s = nxt()
                assert len(s) == p.n
                leaf.append([Pack.CODES[ch] for ch in s])
                phases.append(int(nxt()))
                counts.append(int(nxt()))
            offs.append(offs[-1] + P)
        p.pattern_offsets = np.array(offs, dtype=np.int64)
        p.leafcodes = np.array(leaf, dtype=np.uint8).reshape(-1, p.n)
        p.numPhases = encode_phases(phases)
        p.counts = np.array(counts, dtype=np.int32)
        p.mutRates = np.array(rates)
        return p

    @staticmethod
    def from_control(ctl_path, lib=None, secondary=None, seq_path=None, threads=0):
        """control file + sequence file -> Pack, through the library's own front end
        (gph_control_read / gph_loci_read; the reference's readControlFile / readSeqFile path)"""
        lib = lib or load_library()
        ctl = C.c_void_p()
        rc = lib.gph_control_read(os.fsencode(ctl_path), os.fsencode(secondary) if secondary else None, C.byref(ctl))
        if rc:
            raise ValueError(f"gph_control_read({ctl_path}) failed with status {rc}")
        try:
            cfg, mc, info = GphConfig(), GphMcmcConfig(), GphControlInfo()
            lib.gph_control_get(ctl, C.byref(cfg), C.byref(mc), C.byref(info))
            p = Pack()
            p.n, p.Kc, p.K, p.B, p.rootPop = cfg.n, cfg.Kc, cfg.K, cfg.B, cfg.rootPop
            K, B = p.K, p.B

            def arr(ptr, k, dt):
                return np.array([ptr[i] for i in range(k)], dtype=dt)
            p.samplesPerPop = arr(cfg.samplesPerPop, p.Kc, np.int32)
            p.popFather, p.popSon0, p.popSon1 = (arr(cfg.popFather, K, np.int32), arr(cfg.popSon0, K, np.int32),
                                                 arr(cfg.popSon1, K, np.int32))
            p.bandSrc = arr(cfg.bandSrc, B, np.int32) if B else np.zeros(1, np.int32)
            p.bandTgt = arr(cfg.bandTgt, B, np.int32) if B else np.zeros(1, np.int32)
            p.popName = [lib.gph_control_pop_name(ctl, k).decode() for k in range(K)]
            p.sampleNames = [lib.gph_control_sample_name(ctl, i).decode() for i in range(p.n)]
            for nm in ("thetaAlpha", "thetaBeta", "thetaStart", "ageAlpha", "ageBeta", "ageStart", "sampleAge", "ftTaus"):
                setattr(p, nm, arr(getattr(mc, nm), K, np.float64))
            p.updateSampleAge = arr(mc.updateSampleAge, K, np.int32)
            p.mrAlpha = arr(mc.mrAlpha, B, np.float64) if B else np.zeros(1)
            p.mrBeta = arr(mc.mrBeta, B, np.float64) if B else np.ones(1)
            p.ftCoalTime, p.ftMigTime, p.ftTheta, p.ftMigRate, p.ftMixing = (mc.ftCoalTime, mc.ftMigTime, mc.ftTheta,
                                                                             mc.ftMigRate, mc.ftMixing)
            p.seed, p.startMig, p.doMixing, p.samplesPerLog = mc.seed, mc.startMig, mc.doMixing, mc.samplesPerLog
            p.burnin, p.numSamplesMcmc, p.sampleSkip, p.mutRateMode = (info.burnin, info.numSamples, info.sampleSkip,
                                                                       info.mutRateMode)
            p.varRatesAlpha, p.ftLocusRate = info.varRatesAlpha, info.ftLocusRate
            p.numParameters = mc.numParameters
            p.printFactors = arr(mc.printFactors, p.numParameters, np.float64)
            p.traceFile, p.seqFile = info.traceFile.decode(), info.seqFile.decode()
            loci = C.c_void_p()
            err = C.create_string_buffer(512)
            rc = lib.gph_loci_read(ctl, os.fsencode(seq_path) if seq_path else None, threads, C.byref(loci), err, 512)
            if rc:
                raise ValueError(f"gph_loci_read failed with status {rc}: {err.value.decode()}")
            try:
                L, n = C.c_int64(), C.c_int32()
                po, lf, ph, cn, mr, up = (C.c_void_p() for _ in range(6))
                lib.gph_loci_arrays(loci, C.byref(L), C.byref(n), C.byref(po), C.byref(lf), C.byref(ph), C.byref(cn),
                                    C.byref(mr), C.byref(up))
                p.L = p.numLoci = L.value

                def view(ptr, count, ct, dt):
                    if count == 0:
                        return np.zeros(0, dt)
                    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ct)), shape=(count,)).astype(dt, copy=True)
                p.pattern_offsets = view(po, p.L + 1, C.c_int64, np.int64)
                Ptot = int(p.pattern_offsets[-1])
                p.leafcodes = view(lf, Ptot * p.n, C.c_uint8, np.uint8).reshape(-1, p.n)
                p.numPhases = view(ph, Ptot, C.c_uint16, np.uint16)
                p.counts = view(cn, Ptot, C.c_int32, np.int32)
                p.mutRates = view(mr, p.L, C.c_double, np.float64)
                p.unphased = view(up, p.L, C.c_int32, np.int32)
                p.locusNames = [lib.gph_loci_name(loci, g).decode() for g in range(p.L)]
            finally:
                lib.gph_loci_free(loci)
            return p
        finally:
            lib.gph_control_free(ctl)

    def shard(self, rank, world):
        """contiguous block of ceil(L/world) loci (mirrors OpenMP static scheduling,
        MultiCoreUtils.h:8); returns (begin, end)"""
        per = (self.L + world - 1) // world
        return min(rank * per, self.L), min((rank + 1) * per, self.L)


def summary_table(raw, S, pack):
    """the derived columns of the `-l` summary file from the raw accumulators (README.md): mean = shift + s1 / S,
    var = (s2 - s1 * s1 / S) / (S - 1) for S > 1 (else 0), sd = sqrt(max(var, 0)), pmig = nonzero / S, mean counts = sum / S.
    Keys as the file's header: dataLnL, dataLnL_sd, ..., mig_<src>-><tgt>, pmig_<src>-><tgt>, coal_<pop>[, rate, rate_sd]."""
    t = {"samples": np.full(len(raw["dataLnL.shift"]), S, dtype=np.int64)}

    def moments(q, name):
        sh, s1, s2 = raw[q + ".shift"], raw[q + ".s1"], raw[q + ".s2"]
        with np.errstate(divide="ignore", invalid="ignore"):
            t[name] = sh + s1 / S
            var = (s2 - s1 * s1 / S) / (S - 1) if S > 1 else np.zeros_like(sh)
        t[name + "_sd"] = np.sqrt(np.where(var < 0.0, 0.0, var))
    moments("dataLnL", "dataLnL")
    moments("genLnL", "genLnL")
    moments("tmrca", "tmrca")
    names = getattr(pack, "popName", None) or [str(k) for k in range(pack.K)]
    with np.errstate(divide="ignore", invalid="ignore"):
        for b in range(pack.B):
            band = f"{names[int(pack.bandSrc[b])]}->{names[int(pack.bandTgt[b])]}"
            t["mig_" + band] = raw[f"nmig.{b}"] / S
            t["pmig_" + band] = raw[f"pmig.{b}"] / S
        for k in range(pack.K):
            t["coal_" + names[k]] = raw[f"ncoal.{k}"] / S
    if "rate.shift" in raw:
        moments("rate", "rate")
    return t


GPH_EFULL = -5           # a sampler's _sample found no free row in its device buffer (ancestry _enable: over max_bytes)
COAL_STATS_FULL = GPH_EFULL
COAL_STATS_FIXED = ("iter", "coalStat", "numCoal", "migStat", "numMig", "genLnL", "dataLnL")


def coal_stats_table(rows, n, K, L):
    """the derived statistics of raw coal-stats rows ([samples][7 + 3 * n(n-1)/2 * K], gph_engine_coal_stats_fetch; several
    ranks: their rows added in rank order first), L = loci of all ranks.  One dict per sample: the flat columns as
    printCoalStats prints them (logGenLikelihood = genLnL + dataLnL; logPrior is the caller's) and probCoal = cnt / L,
    probFirstCoal = first / L, meanCoal = agesum / cnt where cnt > 0 else 0 as symmetric (n, n, K) arrays with a zero
    diagonal (patch.c:2256-2266)."""
    iu = np.triu_indices(n, 1)
    npk = n * (n - 1) // 2 * K
    out = []
    for r in np.asarray(rows, dtype=np.float64).reshape(-1, 7 + 3 * npk):
        cnt, first, agesum = (r[7 + b * npk:7 + (b + 1) * npk].reshape(-1, K) for b in range(3))
        d = dict(iter=int(r[0]), coalStat=r[1], numCoal=int(r[2]), migStat=r[3], numMig=int(r[4]),
                 logGenLikelihood=r[5] + r[6], logDataLikelihood=r[6])
        with np.errstate(divide="ignore", invalid="ignore"):
            vals = dict(probCoal=cnt / L, probFirstCoal=first / L, meanCoal=np.where(cnt > 0, agesum / cnt, 0.0))
        for name, v in vals.items():
            m = np.zeros((n, n, K))
            m[iu[0], iu[1], :] = v
            m[iu[1], iu[0], :] = v
            d[name] = m
        out.append(d)
    return out


def _combined(fn, prefix, ranks):
    """(samples, row_doubles) array: the records of the parts of ranks 0..ranks-1 added in rank order"""
    rows, rd = C.c_int64(), C.c_int32()
    if fn(str(prefix).encode(), ranks, None, 0, C.byref(rows), C.byref(rd)):
        raise RuntimeError(f"gphocs_hip: {fn.__name__[4:]} failed")
    out = np.zeros((rows.value, rd.value))
    if rows.value and fn(str(prefix).encode(), ranks, out.ctypes.data_as(C.POINTER(C.c_double)), rows.value, C.byref(rows), C.byref(rd)):
        raise RuntimeError(f"gphocs_hip: {fn.__name__[4:]} failed")
    return out


def coal_stats_combined(lib, prefix, ranks):
    """(samples, row_doubles + 1) array: the records of PREFIX.coal.part<0..ranks-1> added in rank order, logPrior last
    (gph_coal_stats_combined)"""
    return _combined(lib.gph_coal_stats_combined, prefix, ranks)


def time_slices_table(rows, S, K, B):
    """raw time-slices rows ([samples][1 + 2 S (K + B)], gph_engine_time_slices_fetch; several ranks: added in rank order
    first) as one dict per sample: iter, numCoal and deltaT as (K, S) arrays, numMig and migT as (B, S) arrays"""
    out = []
    for r in np.asarray(rows, dtype=np.float64).reshape(-1, 1 + 2 * S * (K + B)):
        cells = r[1:].reshape(K + B, S, 2)
        out.append(dict(iter=int(r[0]), numCoal=cells[:K, :, 0].astype(np.int64), deltaT=cells[:K, :, 1].copy(),
                        numMig=cells[K:, :, 0].astype(np.int64), migT=cells[K:, :, 1].copy()))
    return out


def time_slices_combined(lib, prefix, ranks):
    """(samples, row_doubles) array: the records of PREFIX.slices.part<0..ranks-1> added in rank order
    (gph_time_slices_combined)"""
    return _combined(lib.gph_time_slices_combined, prefix, ranks)


def ancestry_table(raw, S, n, B):
    """the derived columns of PREFIX.loci.tsv from the raw per-locus accumulators (a dict keyed cnt.<b>.<i>, age.<b>.<i>,
    any.<i>, one array entry per locus) after S samples: pAny (L, n) = any / S, p (L, B, n) = cnt / S, age (L, B, n) =
    age_sum / cnt where cnt > 0 else 0 (the genealogy's own units), and keep (L, n) = any > 0, the rows the file prints"""
    L = len(raw["any.0"])
    anyc = np.stack([raw[f"any.{i}"] for i in range(n)], axis=1)
    cnt = np.zeros((L, B, n))
    agesum = np.zeros((L, B, n))
    for b in range(B):
        for i in range(n):
            cnt[:, b, i] = raw[f"cnt.{b}.{i}"]
            agesum[:, b, i] = raw[f"age.{b}.{i}"]
    with np.errstate(divide="ignore", invalid="ignore"):
        return dict(samples=S, pAny=anyc / S, p=cnt / S, age=np.where(cnt > 0, agesum / cnt, 0.0), keep=anyc > 0)


GT_MAX_MIGS = 10         # GPH_GT_MAX_MIGS
GT_OFFSETS = 8           # GPH_GT_O_COUNT


def gene_tree_newick(lib, age, father, left, right, npop, root, mig_branch, mig_band, mig_age, pop_names, band_names, leaf_labels,
                     num_migs=None):
    """one decoded record (the [N] / [10] arrays of Sampler.gene_trees() at one sample and locus) as one line of extended
    Newick (gph_gene_tree_newick: host only).  pop_names / band_names ("<src>-><tgt>") / leaf_labels: lists of str;
    num_migs None: the entries of mig_branch that are not -1.  ValueError for a record that is no tree or a refused name"""
    n = len(leaf_labels)
    f64 = [np.ascontiguousarray(a, dtype=np.float64) for a in (age, mig_age)]
    i32 = [np.ascontiguousarray(a, dtype=np.int32) for a in (father, left, right, npop, mig_branch, mig_band)]
    nm = int(num_migs) if num_migs is not None else int(np.sum(i32[4] >= 0))
    strs = [(C.c_char_p * max(len(v), 1))(*[x.encode() for x in v]) for v in (pop_names, band_names, leaf_labels)]
    args = (n, f64[0].ctypes.data, i32[0].ctypes.data, i32[1].ctypes.data, i32[2].ctypes.data, i32[3].ctypes.data, int(root), nm,
            i32[4].ctypes.data, i32[5].ctypes.data, f64[1].ctypes.data, strs[0], len(pop_names), strs[1], len(band_names), strs[2])
    ln = C.c_size_t()
    rc = lib.gph_gene_tree_newick(*args, None, 0, C.byref(ln))
    if rc == 0:
        buf = C.create_string_buffer(ln.value + 1)
        rc = lib.gph_gene_tree_newick(*args, buf, ln.value + 1, C.byref(ln))
    if rc != 0:
        raise ValueError(f"gphocs_hip: gene_tree_newick refused the record or a name (status {rc})")
    return buf.value.decode()


def clades_consensus(lib, keys, cnt, age, samples, leaf_labels):
    """the majority-rule consensus of one locus's clade table -- keys (P, W), cnt (P), age (P) of Sampler.clades() at one locus,
    over `samples` samples -- as (Newick text, resolved clades) (gph_clades_consensus: host only).  ValueError for a set of
    clades that is no tree or a refused label"""
    n = len(leaf_labels)
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    P, W = keys.shape
    ent = np.zeros((P, W + 2), dtype=np.uint64)
    ent[:, :W] = keys
    ent[:, W] = np.ascontiguousarray(cnt, dtype=np.uint64)
    ent[:, W + 1] = np.ascontiguousarray(age, dtype=np.float64).view(np.uint64)
    labels = (C.c_char_p * max(n, 1))(*[x.encode() for x in leaf_labels])
    ln, res = C.c_size_t(), C.c_int32()
    args = (n, P, ent.ctypes.data, int(samples), labels)
    rc = lib.gph_clades_consensus(*args, None, 0, C.byref(ln), C.byref(res))
    if rc == 0:
        buf = C.create_string_buffer(ln.value + 1)
        rc = lib.gph_clades_consensus(*args, buf, ln.value + 1, C.byref(ln), C.byref(res))
    if rc != 0:
        raise ValueError(f"gphocs_hip: clades_consensus refused the table or a label (status {rc})")
    return buf.value.decode(), res.value


def clades_compare(samplers, min_freq=0.1):
    """the clade tables of R = 2 .. 16 replicate chains compared on the device (gph_engine_clades_compare; samplers[0] leads): a
    dict of loci[Q] (global indices), asdsf[Q], max_sd[Q] (float64) and compared, distinct, shared, dropped [Q] (int64).
    ValueError for what the library refuses (GPH_EARG), RuntimeError for tables that are off or empty (GPH_ESTATE)"""
    samplers = list(samplers)
    R = len(samplers)
    lead = samplers[0] if R else None
    if lead is None or any(s.lib is not lead.lib for s in samplers):
        raise ValueError("gphocs_hip: clades_compare takes samplers of one library")
    Q = lead._clades_shape()[0]
    hs = (C.c_void_p * max(R, 1))(*[s.engine for s in samplers])
    rows = np.zeros((max(Q, 1), 6))
    cnt = C.c_int64()
    rc = lead.lib.gph_engine_clades_compare(hs, R, float(min_freq), rows.ctypes.data_as(C.POINTER(C.c_double)), rows.shape[0], C.byref(cnt))
    if rc == -1:
        raise ValueError("gphocs_hip: clades_compare refused the chains, their tables or min_freq (GPH_EARG)")
    Sampler._chk(rc, "clades_compare")
    rows = rows[:cnt.value]
    out = dict(loci=lead._selected(lead.lib.gph_engine_clades_selected, cnt.value), asdsf=rows[:, 0].copy(), max_sd=rows[:, 1].copy())
    for k, name in enumerate(("compared", "distinct", "shared", "dropped")):
        out[name] = rows[:, 2 + k].astype(np.int64)
    return out


def psrf(x, lib=None):
    """gph_psrf of x[R][S] (R chains, S samples of one quantity): a dict of mean, sd_within, sd_between, psrf.  ValueError for
    fewer than two chains or samples"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError("gphocs_hip: psrf takes x[R][S]")
    o = (C.c_double * 4)()
    rc = (lib or load_library()).gph_psrf(x.ctypes.data_as(C.POINTER(C.c_double)), x.shape[0], x.shape[1], o)
    if rc == -1:
        raise ValueError("gphocs_hip: psrf needs at least two chains of at least two samples (GPH_EARG)")
    Sampler._chk(rc, "psrf")
    return dict(mean=o[0], sd_within=o[1], sd_between=o[2], psrf=o[3])


ESS_SERIES = ("dataLnL", "genLnL", "tmrca", "numMigs", "topo", "rate")      # the series k_ess keeps per locus, in order
ESS_COLUMNS = ("mean", "sd", "tauBatch", "essBatch", "tauAcf", "essAcf", "level", "truncated")


def ess(x, max_lag=0, lib=None):
    """gph_ess of the series x[S]: a dict of mean, sd, tauBatch, essBatch (the batch-sum levels read at the level with
    batch <= sqrt(S)), tauAcf, essAcf (Geyer's initial positive sequence up to max_lag, 0: 2000), level, truncated.  ValueError
    for fewer than two samples"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.ndim != 1:
        raise ValueError("gphocs_hip: ess takes x[S]")
    o = (C.c_double * 8)()
    rc = (lib or load_library()).gph_ess(x.ctypes.data_as(C.POINTER(C.c_double)), x.shape[0], int(max_lag), o)
    if rc == -1:
        raise ValueError("gphocs_hip: ess needs at least two samples (GPH_EARG)")
    Sampler._chk(rc, "ess")
    out = dict(zip(ESS_COLUMNS, list(o)))
    out["level"], out["truncated"] = int(out["level"]), int(out["truncated"])
    return out


def ess_read(a, samples, level=-1, lib=None):
    """gph_ess_read of one series' accumulators a[2 + 2 * 16] over `samples` samples: (mean, sd, tau, ess, level)"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    o = (C.c_double * 5)()
    rc = (lib or load_library()).gph_ess_read(a.ctypes.data_as(C.POINTER(C.c_double)), int(samples), int(level), o)
    if rc == -1:
        raise ValueError("gphocs_hip: ess_read refused the sample count or the level (GPH_EARG)")
    Sampler._chk(rc, "ess_read")
    return o[0], o[1], o[2], o[3], int(o[4])


def _dp(a):
    return np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))


class Sampler:
    """Engine + host MCMC driver for one rank's shard of a Pack."""

    def __init__(self, pack, lib=None, device=0, rank=0, world=1, allreduce=None, comm=None):
        """allreduce: Python hook (gloo tests) -- forces a host synchronisation per reduction point;
        comm: native communicator handle (gph_comm_create_rccl / _shm) -- RCCL runs on the engine's stream"""
        self.lib = lib or load_library(dims=(pack.n, pack.K, pack.B))
        self.pack = pack
        self.rank, self.world = rank, world
        self.begin, self.end = pack.shard(rank, world)
        p = pack
        # a pack that already holds only this rank's loci (bench.py, weak scaling): global_L loci over
        # all ranks, this rank's first locus at global_begin
        L_total, g_begin = p.L, self.begin
        if getattr(p, "global_L", None) is not None:
            L_total, g_begin = int(p.global_L), int(p.global_begin)
            self.begin, self.end = 0, p.L
        self._keep = dict(spp=np.ascontiguousarray(p.samplesPerPop, np.int32),
                          pf=np.ascontiguousarray(p.popFather, np.int32),
                          s0=np.ascontiguousarray(p.popSon0, np.int32),
                          s1=np.ascontiguousarray(p.popSon1, np.int32),
                          bs=np.ascontiguousarray(p.bandSrc, np.int32),
                          bt=np.ascontiguousarray(p.bandTgt, np.int32))
        k = self._keep
        self.cfg = GphConfig(p.n, p.Kc, p.K, p.B, p.rootPop, _ip(k["spp"]), _ip(k["pf"]), _ip(k["s0"]),
                             _ip(k["s1"]), _ip(k["bs"]), _ip(k["bt"]), device, L_total, g_begin)
        self.engine = C.c_void_p()
        self._chk(self.lib.gph_engine_create(C.byref(self.cfg), C.byref(self.engine)), "engine_create")
        self._cb = None
        if allreduce is not None:
            def _cb(user, sums, nsum, mins, nmin):
                try:
                    s = np.ctypeslib.as_array(sums, shape=(nsum,)) if nsum else np.zeros(0)
                    m = np.ctypeslib.as_array(mins, shape=(nmin,)) if nmin else np.zeros(0)
                    allreduce(s, m)
                    return 0
                except Exception as ex:  # pragma: no cover
                    print("allreduce callback failed:", ex)
                    return 1
            self._cb = ALLREDUCE_FN(_cb)
            self._chk(self.lib.gph_engine_set_allreduce(self.engine, self._cb, None), "set_allreduce")
        if comm is not None:
            self._chk(self.lib.gph_engine_set_comm(self.engine, comm), "set_comm")
        b, e = self.begin, self.end
        o0, o1 = p.pattern_offsets[b], p.pattern_offsets[e]
        offs = np.ascontiguousarray(p.pattern_offsets[b:e + 1] - o0, dtype=np.int64)
        leaf = np.ascontiguousarray(p.leafcodes[o0:o1])
        ph = np.ascontiguousarray(p.numPhases[o0:o1], dtype=np.uint16)
        cn = np.ascontiguousarray(p.counts[o0:o1])
        rates = np.ascontiguousarray(p.mutRates[b:e], dtype=np.float64)
        use_rates = bool(np.any(rates != 1.0))
        rc = self.lib.gph_engine_load_loci(self.engine, e - b, offs.ctypes.data, leaf.ctypes.data, ph.ctypes.data, cn.ctypes.data,
                                           rates.ctypes.data if use_rates else None)
        if rc != 0:
            # a refused data set (include/gphocs_hip.h: GPH_LOAD_*): the engine goes, the refusal stays readable
            self.load_error = self.last_error() + (self.lib.gph_engine_last_error_text(self.engine).decode(),)
            self.lib.gph_engine_destroy(self.engine)
            self.engine = None
            err = RuntimeError(f"gphocs_hip: load_loci failed with status {rc}: {self.load_error[2]}")
            err.locus, err.code, err.text = self.load_error
            raise err
        k.update(ta=p.thetaAlpha, tb=p.thetaBeta, ts=p.thetaStart, aa=p.ageAlpha, ab=p.ageBeta,
                 as_=p.ageStart, sa=p.sampleAge, ma=p.mrAlpha, mb=p.mrBeta, ft=p.ftTaus, pf_=p.printFactors,
                 usa=np.ascontiguousarray(getattr(p, "updateSampleAge", np.zeros(p.K, np.int32)), dtype=np.int32))
        self.mcfg = GphMcmcConfig(_dp(k["ta"]), _dp(k["tb"]), _dp(k["ts"]), _dp(k["aa"]), _dp(k["ab"]),
                                  _dp(k["as_"]), _dp(k["sa"]), k["usa"].ctypes.data_as(C.POINTER(C.c_int32)),
                                  _dp(k["ma"]), _dp(k["mb"]),
                                  p.ftCoalTime, p.ftMigTime, p.ftTheta, p.ftMigRate, p.ftMixing,
                                  _dp(k["ft"]), p.seed, p.startMig, p.doMixing, p.samplesPerLog,
                                  p.numParameters, _dp(k["pf_"]),
                                  int(getattr(p, "mutRateMode", 0)) if int(getattr(p, "mutRateMode", 0)) == 1 else 0,
                                  float(getattr(p, "varRatesAlpha", 1.0)), float(getattr(p, "ftLocusRate", -1.0)))
        self.mcmc = C.c_void_p()
        self._chk(self.lib.gph_mcmc_create(self.engine, C.byref(self.cfg), C.byref(self.mcfg),
                                           C.byref(self.mcmc)), "mcmc_create")

    @staticmethod
    def _chk(rc, what):
        if rc != 0:
            raise RuntimeError(f"gphocs_hip: {what} failed with status {rc}")

    def set_record_file(self, path):
        self._chk(self.lib.gph_mcmc_set_record_file(self.mcmc, path.encode() if path else None), "record")

    def initialize(self):
        tc = C.c_int64()
        self._chk(self.lib.gph_mcmc_initialize(self.mcmc, C.byref(tc)), "initialize")
        return tc.value

    def iteration(self, it):
        self._chk(self.lib.gph_mcmc_iteration(self.mcmc, it), f"iteration {it}")

    def set_beta(self, b):
        """power posterior p(D|G)^b p(G|Theta) p(Theta) from the next proposal on (gph_mcmc_set_beta): 1 the posterior, 0 the
        prior; finite, in [0, 64].  Every rank of a chain must be given the same value."""
        self._chk(self.lib.gph_mcmc_set_beta(self.mcmc, float(b)), f"set_beta({b!r})")

    @property
    def beta(self):
        b = C.c_double()
        self._chk(self.lib.gph_mcmc_get_beta(self.mcmc, C.byref(b)), "get_beta")
        return b.value

    def exchange_state(self, other):
        """this chain and `other` exchange their states (gph_mcmc_exchange_state): genealogies, generators, parameters,
        likelihoods.  Each keeps its beta, step sizes, accept counters, record file and samplers."""
        self._chk(self.lib.gph_mcmc_exchange_state(self.mcmc, other.mcmc), "exchange_state")

    def state(self):
        ll, dl = C.c_double(), C.c_double()
        th, ag, mr = np.zeros(self.pack.K), np.zeros(self.pack.K), np.zeros(max(self.pack.B, 1))
        self._chk(self.lib.gph_mcmc_get_state(self.mcmc, C.byref(ll), C.byref(dl), _dp(th), _dp(ag), _dp(mr)),
                  "get_state")
        return dict(logLikelihood=ll.value, dataLogLikelihood=dl.value, theta=th, popAge=ag,
                    migRate=mr[:self.pack.B])

    def dump_state(self, path, with_cond=False):
        self._chk(self.lib.gph_mcmc_dump_state(self.mcmc, path.encode(), int(with_cond)), "dump_state")

    def last_error(self):
        """(global locus index or -1, reference "Fatal Error" code) of the last call that failed with GPH_EKERNEL"""
        g, c = C.c_int64(-1), C.c_int32(0)
        self._chk(self.lib.gph_engine_last_error(self.engine, C.byref(g), C.byref(c)), "last_error")
        return g.value, c.value

    def counters(self, reset=False):
        c = GphCounters()
        self._chk(self.lib.gph_engine_get_counters(self.engine, C.byref(c), int(reset)), "counters")
        return dict(evals=c.evals, eval_nodes=c.eval_nodes, eval_bytes=c.eval_bytes,
                    not_enough_migs=c.not_enough_migs)

    def accept_counts(self):
        a = (C.c_int64 * 9)()
        self._chk(self.lib.gph_mcmc_accept_counts(self.mcmc, a), "accept_counts")
        return list(a)

    def last_kernel_ms(self, which):
        ms = C.c_double()
        self._chk(self.lib.gph_engine_last_kernel_ms(self.engine, which, C.byref(ms)), "kernel_ms")
        return ms.value

    def class_stats(self, which, reset=False):
        o = (C.c_double * 5)()
        self._chk(self.lib.gph_engine_class_stats(self.engine, which, o, int(reset)), "class_stats")
        return dict(launches=o[0], ms=o[1], evals=o[2], bytes=o[3], nodes=o[4])

    def host_stats(self):
        a, b, c, r = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int32()
        self._chk(self.lib.gph_engine_host_stats(self.engine, C.byref(a), C.byref(b), C.byref(c), C.byref(r)), "host_stats")
        return dict(syncs=a.value, collectives=b.value, launches=c.value, resident=bool(r.value))

    def set_timing(self, mask):
        self._chk(self.lib.gph_engine_set_timing(self.engine, mask), "set_timing")

    def unit(self, op, arg=0):
        """kernel-level fixture calls (gph_engine_unit): rows = local loci in input order"""
        stride = max(13, 3 * (self.pack.n - 1), 1 + 5 * (2 * self.pack.n - 1))
        out = np.zeros((self.end - self.begin, stride))
        self._chk(self.lib.gph_engine_unit(self.engine, op, arg, out.ctypes.data_as(C.POINTER(C.c_double)), stride), "unit")
        return out

    def debug_oob(self):
        """(first out-of-range index of a checked build or 0, 1 if the library is a checked build)"""
        w, c = C.c_int32(), C.c_int32()
        self._chk(self.lib.gph_engine_debug_oob(self.engine, C.byref(w), C.byref(c)), "debug_oob")
        return w.value, c.value

    # ---- what the statistics samplers below share
    def _sample(self, fn, what, full, *args):
        rc = fn(self.engine, *args)
        if rc == GPH_EFULL:
            raise BufferError(f"gphocs_hip: the {what} buffer is full; fetch with {full}() first")
        self._chk(rc, fn.__name__[11:])

    def _fetch_rows(self, fn, held, width, dtype=np.float64, with_iters=False, ld=True, extra=()):
        """allocate from the shape, fetch, trim: the rows a sampler took since the last call (the device buffer is emptied).
        ld: the entry point takes the leading dimension of the rows behind them; extra: what else it takes behind those"""
        ct = {np.float64: C.c_double, np.int32: C.c_int32, np.uint64: C.c_uint64}[dtype]
        out = np.zeros((max(held, 1), max(width, 1)), dtype=dtype)
        its = np.zeros(max(held, 1), dtype=np.int32)
        got = C.c_int32()
        args = (its.ctypes.data_as(C.POINTER(C.c_int32)), out.ctypes.data_as(C.POINTER(ct))) + ((out.shape[1],) if ld else ()) if with_iters else \
            (out.ctypes.data_as(C.POINTER(ct)),)
        self._chk(fn(self.engine, *args, *extra, out.shape[0], C.byref(got)), fn.__name__[11:])
        return its[:got.value], out[:got.value]

    @staticmethod
    def _listed(arr, ct=C.c_int64):
        """(pointer, count) of a list an _enable call takes: (None, 0) for None -- with loci: all of this rank --, and a
        non-null pointer for an empty list, which is not the same"""
        if arr is None:
            return None, 0
        keep = arr if len(arr) else np.zeros((1,) + arr.shape[1:], dtype=arr.dtype)
        return keep.ctypes.data_as(C.POINTER(ct)), len(arr)

    def _enabled(self, rc, call, full, refused):
        """the return code of an _enable call over a selection: MemoryError `full` exceed(s) max_bytes, ValueError for what
        the call `refused`, RuntimeError for the rest"""
        if rc == GPH_EFULL:
            raise MemoryError(f"gphocs_hip: {full} max_bytes (GPH_EFULL)")
        if rc == -1:
            raise ValueError(f"gphocs_hip: {call} refused {refused} (GPH_EARG)")
        self._chk(rc, call)

    def _selected(self, fn, Q):
        """this rank's Q selected loci (global indices) as a sampler's _selected entry point hands them out"""
        loci = np.zeros(max(Q, 1), dtype=np.int64)
        cnt = C.c_int64()
        self._chk(fn(self.engine, loci.ctypes.data_as(C.POINTER(C.c_int64)), len(loci), C.byref(cnt)), fn.__name__[11:])
        return loci[:Q].copy()

    def _locus_columns(self, fetch, name, ncol, reset):
        """per-locus columns by name: one array entry per local locus in global locus order"""
        out = np.zeros((self.end - self.begin, max(ncol, 1)))
        self._chk(fetch(self.engine, out.ctypes.data_as(C.POINTER(C.c_double)), out.shape[1], int(bool(reset))), fetch.__name__[11:])
        return {name(c).decode(): out[:, c].copy() for c in range(ncol)}

    # ---- per-locus posterior summaries (gph_engine_locus_summary_*): accumulated on the device, one sample per call
    def enable_locus_summary(self, on=True):
        self._chk(self.lib.gph_engine_locus_summary_enable(self.engine, int(bool(on))), "locus_summary_enable")

    def sample_locus_summary(self):
        self._chk(self.lib.gph_engine_locus_summary_sample(self.engine), "locus_summary_sample")

    def locus_summary(self, raw=False, reset=False):
        """dict of numpy arrays, one entry per local locus in global locus order.  raw=True: the accumulators as the engine
        keeps them, keyed by their machine names (gph_engine_locus_summary_column_name) + "samples".  raw=False: the columns
        of the `-l` summary file (README.md), derived from the raw ones with the formulas given there."""
        nc, ns = C.c_int32(), C.c_int64()
        self._chk(self.lib.gph_engine_locus_summary_columns(self.engine, C.byref(nc), C.byref(ns)), "locus_summary_columns")
        cols = self._locus_columns(self.lib.gph_engine_locus_summary_fetch,
                                   lambda c: self.lib.gph_engine_locus_summary_column_name(self.engine, c), nc.value, reset)
        S = ns.value
        if raw:
            cols["samples"] = np.full(self.end - self.begin, S, dtype=np.int64)
            return cols
        return summary_table(cols, S, self.pack)

    # ---- genome-wide coalescent / sample-pair statistics per sample (gph_engine_coal_stats_*): one row per call, on the device
    def enable_coal_stats(self, capacity, chunk=0):
        """a device buffer of `capacity` samples; 0 switches the feature off and frees it.  chunk (tests): slots per chunk of
        the kernel, 0 = the default"""
        self._chk(self.lib.gph_engine_coal_stats_set_chunk(self.engine, int(chunk)), "coal_stats_set_chunk")
        self._chk(self.lib.gph_engine_coal_stats_enable(self.engine, int(capacity)), "coal_stats_enable")

    def sample_coal_stats(self, it):
        """one sample of the current state, labelled iteration `it`; BufferError when the device buffer is full"""
        self._sample(self.lib.gph_engine_coal_stats_sample, "coal-stats", "coal_stats", int(it))

    def coal_stats(self, raw=False):
        """the samples taken since the last call (the device buffer is emptied).  raw=True: the rows as the engine keeps them,
        a (samples, row_doubles) array over THIS rank's loci (columns: gph_engine_coal_stats_column_name).  raw=False: a list
        of dicts, one per sample (coal_stats_table); several ranks must add their raw rows in rank order first."""
        rd, fill, n, K = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        self._chk(self.lib.gph_engine_coal_stats_shape(self.engine, C.byref(rd), C.byref(fill), C.byref(n), C.byref(K)), "coal_stats_shape")
        out = self._fetch_rows(self.lib.gph_engine_coal_stats_fetch, fill.value, rd.value)[1]
        if raw:
            return out
        L = int(getattr(self.pack, "global_L", None) or self.pack.L)
        return coal_stats_table(out, n.value, K.value, L)

    def coal_stats_columns(self):
        rd = C.c_int32()
        self._chk(self.lib.gph_engine_coal_stats_shape(self.engine, C.byref(rd), None, None, None), "coal_stats_shape")
        return [self.lib.gph_engine_coal_stats_column_name(self.engine, c).decode() for c in range(rd.value)]

    # ---- coalescence / migration statistics per time slice (gph_engine_time_slices_*): one row per call, on the device
    def enable_time_slices(self, slices, capacity, chunk=0):
        """a device buffer of `capacity` samples of `slices` slices per branch and band; capacity 0 switches the feature off.
        chunk (tests): slots per chunk of the kernel, 0 = the default.  ValueError for a slice count out of range"""
        self._chk(self.lib.gph_engine_time_slices_set_chunk(self.engine, int(chunk)), "time_slices_set_chunk")
        rc = self.lib.gph_engine_time_slices_enable(self.engine, int(slices), int(capacity))
        if rc == -1 and capacity > 0:
            raise ValueError(f"gphocs_hip: time_slices_enable refused slices={slices}, capacity={capacity} (GPH_EARG)")
        self._chk(rc, "time_slices_enable")

    def sample_time_slices(self, it):
        """one sample of the current state, labelled iteration `it`; BufferError when the device buffer is full"""
        self._sample(self.lib.gph_engine_time_slices_sample, "time-slices", "time_slices", int(it))

    def _time_slices_shape(self):
        v = [C.c_int32() for _ in range(6)]
        self._chk(self.lib.gph_engine_time_slices_shape(self.engine, *[C.byref(x) for x in v]), "time_slices_shape")
        return [x.value for x in v]

    def time_slices_staged_bytes(self):
        """bytes of a page k_time_slices copies into LDS per locus and sample"""
        return self._time_slices_shape()[5]

    def time_slices(self, raw=True):
        """the samples taken since the last call (the device buffer is emptied).  raw=True: a (samples, 1 + 2 S (K + B)) array
        over THIS rank's loci (columns: time_slices_columns()); raw=False: a list of dicts (time_slices_table)"""
        rd, fill, S, K, B, _ = self._time_slices_shape()
        out = self._fetch_rows(self.lib.gph_engine_time_slices_fetch, fill, rd)[1]
        return out if raw else time_slices_table(out, S, K, B)

    def time_slices_columns(self):
        rd = self._time_slices_shape()[0]
        return [self.lib.gph_engine_time_slices_column_name(self.engine, c).decode() for c in range(rd)]

    # ---- per-locus, per-sample migration ancestry (gph_engine_ancestry_*): accumulated on the device, one sample per call
    def enable_ancestry(self, capacity, max_bytes=0):
        """per-locus accumulators and a device buffer of `capacity` per-sample rows; capacity 0 switches the feature off.
        MemoryError when the accumulators would exceed max_bytes (0: 1 GiB); the sampler stays usable"""
        rc = self.lib.gph_engine_ancestry_enable(self.engine, int(capacity), int(max_bytes))
        if rc == GPH_EFULL:
            raise MemoryError("gphocs_hip: the ancestry accumulators exceed max_bytes (GPH_EFULL)")
        self._chk(rc, "ancestry_enable")

    def sample_ancestry(self, it):
        """one sample of the current state, labelled iteration `it`; BufferError when the row buffer is full"""
        self._sample(self.lib.gph_engine_ancestry_sample, "ancestry row", "ancestry_rows", int(it))

    def _ancestry_shape(self):
        nc, ri, ns, held = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32()
        self._chk(self.lib.gph_engine_ancestry_shape(self.engine, C.byref(nc), C.byref(ri), C.byref(ns), C.byref(held)), "ancestry_shape")
        return nc.value, ri.value, ns.value, held.value

    def ancestry_loci(self, raw=False, reset=False):
        """one entry per local locus in global locus order.  raw=True: a dict of the accumulators as the engine keeps them,
        keyed by their machine names (cnt.<b>.<i>, age.<b>.<i>, any.<i>) + "samples".  raw=False: ancestry_table of them"""
        nc, _, S, _ = self._ancestry_shape()
        cols = self._locus_columns(self.lib.gph_engine_ancestry_fetch_loci,
                                   lambda c: self.lib.gph_engine_ancestry_column_name(self.engine, 0, c), nc, reset)
        if raw:
            cols["samples"] = np.full(self.end - self.begin, S, dtype=np.int64)
            return cols
        return ancestry_table(cols, S, self.pack.n, self.pack.B)

    def ancestry_rows(self):
        """(iterations, rows): the per-sample rows taken since the last call, an int32 (samples, n (B + 1)) array over THIS
        rank's loci -- any.<i>, then hit.<b>.<i> -- and their iterations; the device buffer is emptied"""
        _, ri, _, held = self._ancestry_shape()
        its, out = self._fetch_rows(self.lib.gph_engine_ancestry_fetch_rows, held, ri, np.int32, with_iters=True)
        return its, out[:, :ri]

    # ---- sampled genealogies of selected loci (gph_engine_gene_trees_*): gathered on the device, one row of records per call
    def enable_gene_trees(self, capacity, loci=None, max_bytes=0):
        """a device buffer of `capacity` samples of the selected loci (global 0-based indices, strictly increasing; None:
        all loci of this rank; indices of other ranks' blocks are ignored); capacity 0 switches the feature off.  ValueError
        for a negative index or a list that is not increasing, MemoryError when the buffer would exceed max_bytes (0: 256 MB)"""
        sel = self._listed(None if loci is None else np.ascontiguousarray(loci, dtype=np.int64))
        self._enabled(self.lib.gph_engine_gene_trees_enable(self.engine, int(capacity), *sel, int(max_bytes)), "gene_trees_enable",
                      "the gene-trees row buffer exceeds", "the capacity or the selection")

    def sample_gene_trees(self, it):
        """one sample of the current state, labelled iteration `it`; BufferError when the row buffer is full"""
        self._sample(self.lib.gph_engine_gene_trees_sample, "gene-trees", "gene_trees", int(it))

    def _gene_trees_shape(self):
        q, N, rb, held = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32()
        off = (C.c_int32 * GT_OFFSETS)()
        self._chk(self.lib.gph_engine_gene_trees_shape(self.engine, C.byref(q), C.byref(N), C.byref(rb), off, C.byref(held)), "gene_trees_shape")
        return q.value, N.value, rb.value, off, held.value

    def gene_trees(self, raw=False):
        """the samples taken since the last call (the device buffer is emptied), S samples of this rank's Q selected loci: a
        dict of iters[S], loci[Q] (global indices), age / father / left / right / npop [S, Q, N], root / num_migs / dataLnL /
        genLnL [S, Q], and the live migrations in `living` order, mig_branch / mig_band / mig_spop / mig_tpop / mig_age
        [S, Q, 10] (-1 and age 0 beyond num_migs).  raw=True adds records: the bytes as fetched, uint8 [S, Q, record_bytes]"""
        Q, N, rb, off, held = self._gene_trees_shape()
        loci = self._selected(self.lib.gph_engine_gene_trees_selected, Q)
        buf = np.zeros((max(held, 1), max(Q * rb, 1)), dtype=np.uint8)
        its = np.zeros(max(held, 1), dtype=np.int32)
        got = C.c_int32()
        self._chk(self.lib.gph_engine_gene_trees_fetch(self.engine, its.ctypes.data_as(C.POINTER(C.c_int32)), buf.ctypes.data, buf.shape[0],
                                                       C.byref(got)), "gene_trees_fetch")
        S, M = got.value, GT_MAX_MIGS
        rec = np.ascontiguousarray(buf[:S, :Q * rb]).reshape(S, Q, rb)
        out = dict(iters=its[:S].copy(), loci=loci)
        shapes = dict(age=((S, Q, N), np.float64), father=((S, Q, N), np.int32), left=((S, Q, N), np.int32), right=((S, Q, N), np.int32),
                      npop=((S, Q, N), np.int32), root=((S, Q), np.int32), num_migs=((S, Q), np.int32), dataLnL=((S, Q), np.float64),
                      genLnL=((S, Q), np.float64), mig_branch=((S, Q, M), np.int32), mig_band=((S, Q, M), np.int32),
                      mig_spop=((S, Q, M), np.int32), mig_tpop=((S, Q, M), np.int32), mig_age=((S, Q, M), np.float64))
        for k, (shp, dt) in shapes.items():
            out[k] = np.zeros(shp, dtype=dt)
        if S * Q:
            self._chk(self.lib.gph_gene_trees_decode(rec.ctypes.data, S * Q, rb, off, N, *[out[k].ctypes.data for k in shapes]), "gene_trees_decode")
        if raw:
            out["records"] = rec
        return out

    # ---- clade tables of selected loci (gph_engine_clades_*): accumulated on the device, one sample per call
    def enable_clades(self, slots=0, loci=None, max_bytes=0):
        """per-locus clade tables of `slots` physical slots (a power of two; 0: the smallest one >= 8 (n - 1)) for the selected
        loci (as enable_gene_trees; None: all loci of this rank).  ValueError for refused slots or a refused selection,
        MemoryError when the tables would exceed max_bytes (0: 1 GiB); the sampler stays usable"""
        sel = self._listed(None if loci is None else np.ascontiguousarray(loci, dtype=np.int64))
        self._enabled(self.lib.gph_engine_clades_enable(self.engine, int(slots), *sel, int(max_bytes)), "clades_enable",
                      "the clade tables exceed", "the slots or the selection")

    def sample_clades(self):
        """one sample of the current state into the tables"""
        self._chk(self.lib.gph_engine_clades_sample(self.engine), "clades_sample")

    def _clades_shape(self):
        q, P, W, lim, S = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        self._chk(self.lib.gph_engine_clades_shape(self.engine, C.byref(q), C.byref(P), C.byref(W), C.byref(lim), C.byref(S)), "clades_shape")
        return q.value, P.value, W.value, lim.value, S.value

    def clades(self, reset=False):
        """the tables of this rank's Q selected loci as the device holds them: a dict of loci[Q] (global indices), samples,
        slots (P), words (W), limit, nkeys[Q], dropped[Q], keys (Q, P, W) uint64, cnt (Q, P) uint64 (0: an empty slot) and
        age (Q, P) float64 (the age sums).  reset=True zeroes tables, header words and the sample count afterwards"""
        Q, P, W, lim, S = self._clades_shape()
        loci = self._selected(self.lib.gph_engine_clades_selected, Q)
        ent = np.zeros((max(Q, 1), max(P, 1), W + 2), dtype=np.uint64)
        nk, dr = np.zeros(max(Q, 1), dtype=np.uint32), np.zeros(max(Q, 1), dtype=np.uint32)
        self._chk(self.lib.gph_engine_clades_fetch(self.engine, ent.ctypes.data, nk.ctypes.data, dr.ctypes.data, int(bool(reset))), "clades_fetch")
        ent = ent[:Q, :P]
        return dict(loci=loci, samples=S, slots=P, words=W, limit=lim, nkeys=nk[:Q].copy(), dropped=dr[:Q].copy(),
                    keys=ent[:, :, :W].copy(), cnt=ent[:, :, W].copy(), age=ent[:, :, W + 1].copy().view(np.float64))

    # ---- effective sample sizes of selected loci (gph_engine_ess_*): accumulated on the device, one sample per call
    def ess_enable(self, loci=None, max_bytes=0):
        """the batch-sum levels of dataLnL, genLnL, tmrca, numMigs, topo (and rate under locus-mut-rate VAR) for the selected
        loci (as enable_gene_trees; None: all loci of this rank).  ValueError for a refused selection, MemoryError when the
        accumulators would exceed max_bytes (0: 1 GiB); the sampler stays usable"""
        sel = self._listed(None if loci is None else np.ascontiguousarray(loci, dtype=np.int64))
        self._enabled(self.lib.gph_engine_ess_enable(self.engine, *sel, int(max_bytes)), "ess_enable", "the ESS accumulators exceed", "the selection")

    def ess_sample(self):
        """one sample of the current state into the accumulators"""
        self._chk(self.lib.gph_engine_ess_sample(self.engine), "ess_sample")

    def _ess_shape(self):
        q, M, J, W, S = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        self._chk(self.lib.gph_engine_ess_shape(self.engine, C.byref(q), C.byref(M), C.byref(J), C.byref(W), C.byref(S)), "ess_shape")
        return q.value, M.value, J.value, W.value, S.value

    def ess(self, reset=False, level=-1):
        """the accumulators of this rank's Q selected loci as the device holds them and their read-out: a dict of loci[Q]
        (global indices), samples, series (names, M of them), levels (J), words (W), acc (Q, M, 2 + 2J) float64, changes[Q]
        uint32, focal (Q, n - 1, W) uint64, and the table -- mean, sd, tau, ess (Q, M) float64 and `level` (gph_ess_read of every
        series at `level`, -1: batch <= sqrt(samples)) -- with min_ess[Q]: the smallest ess over the series that were not
        constant (0 when all were).  reset=True zeroes everything and the sample count afterwards"""
        Q, M, J, W, S = self._ess_shape()
        if M == 0:
            raise RuntimeError("gphocs_hip: ess: not enabled (GPH_ESTATE)")
        loci = self._selected(self.lib.gph_engine_ess_selected, Q)
        ni = max(self.pack.n - 1, 0)
        acc = np.zeros((max(Q, 1), M, 2 + 2 * J), dtype=np.float64)
        changes, focal = np.zeros(max(Q, 1), dtype=np.uint32), np.zeros((max(Q, 1), ni, W), dtype=np.uint64)
        self._chk(self.lib.gph_engine_ess_fetch(self.engine, acc.ctypes.data, changes.ctypes.data, focal.ctypes.data if focal.size else None,
                                                int(bool(reset))), "ess_fetch")
        acc, changes, focal = acc[:Q], changes[:Q], focal[:Q]
        tab = np.zeros((4, Q, M), dtype=np.float64)
        used = ess_read(np.zeros(2 + 2 * J), S, level, self.lib)[4]
        for q in range(Q):
            for m in range(M):
                tab[:, q, m] = ess_read(acc[q, m], S, level, self.lib)[:4]
        moved = tab[1] > 0.0
        min_ess = np.where(moved.any(axis=1), np.where(moved, tab[3], np.inf).min(axis=1), 0.0) if Q else np.zeros(0)
        return dict(loci=loci, samples=S, series=ESS_SERIES[:M], levels=J, words=W, acc=acc.copy(), changes=changes.copy(),
                    focal=focal.copy(), mean=tab[0], sd=tab[1], tau=tab[2], ess=tab[3], level=used, min_ess=min_ess)

    # ---- posterior predictive checks of selected loci (gph_engine_predictive_*): simulated on the device, one sample per call
    def predictive_enable(self, seed, capacity, loci=None, max_bytes=0):
        """per-locus accumulators of the replicate statistics for the selected loci (as enable_gene_trees; None: all loci of
        this rank) and a device buffer of `capacity` per-sample rows; capacity 0 switches the feature off.  The replicates are
        a pure function of (seed, locus, sample, site, node).  ValueError for a refused selection or a locus whose statistics
        do not fit 32 bits, MemoryError when accumulators and rows would exceed max_bytes (0: 1 GiB); the sampler stays usable"""
        sel = self._listed(None if loci is None else np.ascontiguousarray(loci, dtype=np.int64))
        self._enabled(self.lib.gph_engine_predictive_enable(self.engine, int(seed) & 0xffffffffffffffff, int(capacity), *sel, int(max_bytes)),
                      "predictive_enable", "the predictive accumulators and rows exceed", "the capacity, the selection or a locus")

    def predictive_sample(self, it):
        """one replicate of every selected locus under the current state, labelled iteration `it`; BufferError when the row
        buffer is full"""
        self._sample(self.lib.gph_engine_predictive_sample, "predictive row", "predictive_rows", int(it))

    def _predictive_shape(self):
        q, c, S, held = C.c_int64(), C.c_int32(), C.c_int64(), C.c_int32()
        self._chk(self.lib.gph_engine_predictive_shape(self.engine, C.byref(q), C.byref(c), C.byref(S), C.byref(held)), "predictive_shape")
        return q.value, c.value, S.value, held.value

    def predictive_columns(self):
        return [self.lib.gph_engine_predictive_column_name(self.engine, c).decode() for c in range(self._predictive_shape()[1])]

    def predictive(self, reset=False):
        """the accumulators of this rank's Q selected loci as the device holds them: a dict of loci[Q] (global indices), samples,
        stats (the C names), sites[Q] and acc (Q, C, 5) float64 -- obs, gt, eq, s1, s2.  reset=True zeroes them afterwards and
        restarts the sample count"""
        Q, nc, S, _ = self._predictive_shape()
        if nc == 0:
            raise RuntimeError("gphocs_hip: predictive: not enabled (GPH_ESTATE)")
        loci = self._selected(self.lib.gph_engine_predictive_selected, Q)
        names = self.predictive_columns()
        acc, sites = np.zeros((max(Q, 1), nc, 5), dtype=np.float64), np.zeros(max(Q, 1), dtype=np.int64)
        self._chk(self.lib.gph_engine_predictive_fetch_loci(self.engine, acc.ctypes.data, sites.ctypes.data, int(bool(reset))), "predictive_fetch_loci")
        return dict(loci=loci, samples=S, stats=names, sites=sites[:Q].copy(), acc=acc[:Q].copy())

    def predictive_rows(self):
        """(iterations, rows, observed): the per-sample rows taken since the last call, a uint64 (samples, C) array of the
        replicate totals over THIS rank's selected loci, their iterations, and the data's totals observed[C]; the device
        buffer is emptied"""
        _, nc, _, held = self._predictive_shape()
        if nc == 0:
            raise RuntimeError("gphocs_hip: predictive_rows: not enabled (GPH_ESTATE)")
        obs = np.zeros(nc, dtype=np.uint64)
        its, rows = self._fetch_rows(self.lib.gph_engine_predictive_fetch_rows, held, nc, np.uint64, with_iters=True, ld=False, extra=(obs.ctypes.data,))
        return its.copy(), rows.copy(), obs

    # ---- triplet topology weights of selected loci (gph_engine_triplets_*): accumulated on the device, one sample per call
    def triplets_enable(self, capacity, loci=None, triples=None, max_bytes=0):
        """per-locus accumulators W, A of every (triple, topology) slot for the selected loci (as enable_gene_trees; None: all
        loci of this rank) and a device buffer of `capacity` per-sample rows; capacity 0 switches the feature off.  triples:
        None = every triple P < Q < R of current populations with samples, else a list of (P, Q, R) population indices in any
        order.  ValueError for a refused selection or triple list (stderr names the cause; the sampler is left as it was),
        MemoryError when accumulators and rows would exceed max_bytes (0: 1 GiB)"""
        sel = self._listed(None if loci is None else np.ascontiguousarray(loci, dtype=np.int64))
        tri = self._listed(None if triples is None else np.ascontiguousarray(triples, dtype=np.int32).reshape(-1, 3), C.c_int32)
        self._enabled(self.lib.gph_engine_triplets_enable(self.engine, int(capacity), *sel, *tri, int(max_bytes)), "triplets_enable",
                      "the triplets accumulators and rows exceed", "the capacity, the selection or the triples")

    def triplets_sample(self, it):
        """the weights of every selected locus under the current state, labelled iteration `it`; BufferError when the row
        buffer is full"""
        self._sample(self.lib.gph_engine_triplets_sample, "triplets row", "triplets_rows", int(it))

    def _triplets_shape(self):
        t, sl, q, S, held = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64(), C.c_int32()
        self._chk(self.lib.gph_engine_triplets_shape(self.engine, C.byref(t), C.byref(sl), C.byref(q), C.byref(S), C.byref(held)), "triplets_shape")
        return t.value, sl.value, q.value, S.value, held.value

    def triplets_columns(self):
        return [self.lib.gph_engine_triplets_column_name(self.engine, c).decode() for c in range(self._triplets_shape()[1])]

    def triplets(self, reset=False):
        """the accumulators of this rank's Q selected loci as the device holds them: a dict of loci[Q] (global indices), samples,
        slots (the 3 T names "<X>,<Y>|<Z>", population indices), triples (T, 3), W and A (Q, T, 3) float64.  reset=True zeroes
        them afterwards and restarts the sample count"""
        T, slots, Q, S, _ = self._triplets_shape()
        if slots == 0:
            raise RuntimeError("gphocs_hip: triplets: not enabled (GPH_ESTATE)")
        loci = self._selected(self.lib.gph_engine_triplets_selected, Q)
        names = self.triplets_columns()
        acc = np.zeros((max(Q, 1), 2, T, 3), dtype=np.float64)
        self._chk(self.lib.gph_engine_triplets_fetch_loci(self.engine, acc.ctypes.data, 2 * slots, int(bool(reset))), "triplets_fetch_loci")
        triples = np.array([[int(x) for x in nm.replace("|", ",").split(",")] for nm in names[0::3]], dtype=np.int32).reshape(T, 3)
        return dict(loci=loci, samples=S, slots=names, triples=triples, W=acc[:Q, 0].copy(), A=acc[:Q, 1].copy())

    def triplets_rows(self):
        """(iterations, rows): the per-sample rows taken since the last call, a uint64 (samples, 3 T) array of the totals of cnt
        over THIS rank's selected loci, and their iterations; the device buffer is emptied"""
        _, slots, _, _, held = self._triplets_shape()
        if slots == 0:
            raise RuntimeError("gphocs_hip: triplets_rows: not enabled (GPH_ESTATE)")
        its, rows = self._fetch_rows(self.lib.gph_engine_triplets_fetch_rows, held, slots, np.uint64, with_iters=True)
        return its.copy(), rows.copy()

    # ---- expected substitutions per population branch and per sample (gph_engine_mutations_*): accumulated on the device
    def mutations_enable(self, capacity, loci=None, max_bytes=0):
        """per-locus accumulators of mut_p / exp_p (every population) and mutExt_i / expExt_i (every leaf) for the selected loci
        (as enable_gene_trees; None: all loci of this rank) and a device buffer of `capacity` per-sample rows; capacity 0 switches
        the feature off.  ValueError for a refused selection (stderr names the cause; the sampler is left as it was), MemoryError
        when accumulators and rows would exceed max_bytes (0: 1 GiB)"""
        sel = self._listed(None if loci is None else np.ascontiguousarray(loci, dtype=np.int64))
        self._enabled(self.lib.gph_engine_mutations_enable(self.engine, int(capacity), *sel, int(max_bytes)), "mutations_enable",
                      "the mutations accumulators and rows exceed", "the capacity or the selection")

    def mutations_sample(self, it):
        """the expected substitutions of every selected locus under the current state, labelled iteration `it`; BufferError when
        the row buffer is full"""
        self._sample(self.lib.gph_engine_mutations_sample, "mutations row", "mutations_rows", int(it))

    def _mutations_shape(self):
        c, ch, q, S, held = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64(), C.c_int32()
        self._chk(self.lib.gph_engine_mutations_shape(self.engine, C.byref(c), C.byref(ch), C.byref(q), C.byref(S), C.byref(held)), "mutations_shape")
        return c.value, ch.value, q.value, S.value, held.value

    def mutations_columns(self):
        return [self.lib.gph_engine_mutations_column_name(self.engine, c).decode() for c in range(self._mutations_shape()[0])]

    def mutations(self, reset=False):
        """the accumulators of this rank's Q selected loci as the device holds them: a dict of loci[Q] (global indices), samples,
        chunk (the selected loci a partial row sums), columns (the C names) and mut, exp (Q, K), mutExt, expExt (Q, n) float64: the
        sums over the samples.  reset=True zeroes them afterwards and restarts the sample count"""
        Cn, chunk, Q, S, _ = self._mutations_shape()
        if Cn == 0:
            raise RuntimeError("gphocs_hip: mutations: not enabled (GPH_ESTATE)")
        loci = self._selected(self.lib.gph_engine_mutations_selected, Q)
        acc = np.zeros((max(Q, 1), Cn), dtype=np.float64)
        self._chk(self.lib.gph_engine_mutations_fetch_loci(self.engine, acc.ctypes.data, Cn, int(bool(reset))), "mutations_fetch_loci")
        K, n = self.pack.K, self.pack.n
        acc = acc[:Q]
        return dict(loci=loci, samples=S, chunk=chunk, columns=self.mutations_columns(), mut=acc[:, :K].copy(), exp=acc[:, K:2 * K].copy(),
                    mutExt=acc[:, 2 * K:2 * K + n].copy(), expExt=acc[:, 2 * K + n:].copy())

    def mutations_rows(self):
        """(iterations, rows): the per-sample rows taken since the last call, a float64 (samples, C) array of the columns summed over
        THIS rank's selected loci, and their iterations; the device buffer is emptied"""
        Cn, _, _, _, held = self._mutations_shape()
        if Cn == 0:
            raise RuntimeError("gphocs_hip: mutations_rows: not enabled (GPH_ESTATE)")
        _, rows = self._fetch_rows(self.lib.gph_engine_mutations_fetch_rows, held, 1 + Cn)
        return rows[:, 0].astype(np.int32), rows[:, 1:].copy()

    # ---- pairwise coalescence-time distributions of selected loci (gph_engine_pair_times_*): accumulated on the device
    def pair_times_enable(self, capacity, edges, loci=None, pairs=None, max_bytes=0):
        """per-locus accumulators A, Y, X, M of every pair slot for the selected loci (as enable_gene_trees; None: all loci of this
        rank) and a device buffer of `capacity` per-sample rows; capacity 0 switches the feature off.  edges: the E increasing,
        finite, positive edges of the time grid (B = E + 1 bins).  pairs: None = every pair P <= Q of current populations with a
        leaf pair, else a list of (P, Q) population indices in any order.  ValueError for a refused selection, pair list or grid
        (stderr names the cause; the sampler is left as it was), MemoryError when accumulators and rows would exceed max_bytes
        (0: 1 GiB)"""
        sel = self._listed(None if loci is None else np.ascontiguousarray(loci, dtype=np.int64))
        pr = self._listed(None if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2), C.c_int32)
        ed = self._listed(np.ascontiguousarray(edges, dtype=np.float64).reshape(-1), C.c_double)
        self._enabled(self.lib.gph_engine_pair_times_enable(self.engine, int(capacity), *sel, *pr, *ed, int(max_bytes)), "pair_times_enable",
                      "the pair-times accumulators and rows exceed", "the capacity, the selection, the pairs or the grid")

    def pair_times_sample(self, it):
        """the distributions of every selected locus under the current state, labelled iteration `it`; BufferError when the row
        buffer is full"""
        self._sample(self.lib.gph_engine_pair_times_sample, "pair-times row", "pair_times_rows", int(it))

    def _pair_times_shape(self):
        """(NP, B, G, selected, samples, rows held)"""
        a, b, g, q, S, held = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64(), C.c_int32()
        self._chk(self.lib.gph_engine_pair_times_shape(self.engine, C.byref(a), C.byref(b), C.byref(g), C.byref(q), C.byref(S), C.byref(held), None),
                  "pair_times_shape")
        return a.value, b.value, g.value, q.value, S.value, held.value

    def pair_times_columns(self):
        NP, B = self._pair_times_shape()[:2]
        return [self.lib.gph_engine_pair_times_column_name(self.engine, c).decode() for c in range(NP * (B + 2))]

    def pair_times(self, reset=False):
        """the accumulators of this rank's Q selected loci as the device holds them: a dict of loci[Q] (global indices), pairs
        (NP, 2) population indices, edges[E] as given, samples, and A, Y, X, M (Q, NP) float64.  reset=True zeroes them afterwards
        and restarts the sample count"""
        NP, B, _, Q, S, _ = self._pair_times_shape()
        if NP == 0:
            raise RuntimeError("gphocs_hip: pair_times: not enabled (GPH_ESTATE)")
        loci = self._selected(self.lib.gph_engine_pair_times_selected, Q)
        edges = np.zeros(B - 1, dtype=np.float64)
        self._chk(self.lib.gph_engine_pair_times_shape(self.engine, None, None, None, None, None, None, edges.ctypes.data), "pair_times_shape")
        names = [self.lib.gph_engine_pair_times_column_name(self.engine, NP * B + k).decode() for k in range(NP)]
        pairs = np.array([[int(x) for x in nm[len("below_"):].split("|")] for nm in names], dtype=np.int32).reshape(NP, 2)
        acc = np.zeros((max(Q, 1), 4, NP), dtype=np.float64)
        self._chk(self.lib.gph_engine_pair_times_fetch_loci(self.engine, acc.ctypes.data, 4 * NP, int(bool(reset))), "pair_times_fetch_loci")
        return dict(loci=loci, pairs=pairs, edges=edges, samples=S, A=acc[:Q, 0].copy(), Y=acc[:Q, 1].copy(), X=acc[:Q, 2].copy(), M=acc[:Q, 3].copy())

    def pair_times_rows(self):
        """(iterations, rows): the per-sample rows taken since the last call, a uint64 (samples, NP (B + 2)) array over THIS rank's
        selected loci -- per slot the B histogram totals, then per slot the pairs below the split, then per slot the loci with
        one --, and their iterations; the device buffer is emptied"""
        NP, B, _, _, _, held = self._pair_times_shape()
        if NP == 0:
            raise RuntimeError("gphocs_hip: pair_times_rows: not enabled (GPH_ESTATE)")
        its, rows = self._fetch_rows(self.lib.gph_engine_pair_times_fetch_rows, held, NP * (B + 2), np.uint64, with_iters=True)
        return its.copy(), rows.copy()

    # ---- site-frequency spectra, data against sampled genealogies (gph_engine_sfs_*): accumulated on the device
    def sfs_enable(self, capacity, loci=None, pairs=None, max_bytes=0):
        """per-locus accumulators E of every slot -- the folded spectrum bins of every current population with two leaves, then
        privP, privQ, shared, fixed of every pair -- for the selected loci (as enable_gene_trees; None: all loci of this rank), the
        data side (obs, use, sites: formed once, here) and a device buffer of `capacity` per-sample rows; capacity 0 switches the
        feature off.  pairs: None = every pair P < Q of current populations with samples, [] = none, else a list of (P, Q)
        population indices in any order.  ValueError for a refused selection or pair list (stderr names the cause; the sampler is
        left as it was), MemoryError when accumulators and rows would exceed max_bytes (0: 1 GiB)"""
        sel = self._listed(None if loci is None else np.ascontiguousarray(loci, dtype=np.int64))
        pr = self._listed(None if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2), C.c_int32)
        self._enabled(self.lib.gph_engine_sfs_enable(self.engine, int(capacity), *sel, *pr, int(max_bytes)), "sfs_enable",
                      "the sfs accumulators and rows exceed", "the capacity, the selection or the pairs")

    def sfs_sample(self, it):
        """the expected spectra of every selected locus under the current state, labelled iteration `it`; BufferError when the row
        buffer is full"""
        self._sample(self.lib.gph_engine_sfs_sample, "sfs row", "sfs_rows", int(it))

    def _sfs_shape(self):
        """(NS, NG, G, selected, samples, rows held)"""
        a, b, g, q, S, held = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64(), C.c_int32()
        self._chk(self.lib.gph_engine_sfs_shape(self.engine, C.byref(a), C.byref(b), C.byref(g), C.byref(q), C.byref(S), C.byref(held)), "sfs_shape")
        return a.value, b.value, g.value, q.value, S.value, held.value

    def sfs_columns(self):
        """the NS slot names"""
        return [self.lib.gph_engine_sfs_column_name(self.engine, c).decode() for c in range(self._sfs_shape()[0])]

    def _sfs_tables(self):
        NS, NG = self._sfs_shape()[:2]
        if NS == 0:
            raise RuntimeError("gphocs_hip: sfs: not enabled (GPH_ESTATE)")
        slots = np.zeros((NS, 5), dtype=np.int32)
        self._chk(self.lib.gph_engine_sfs_slots(self.engine, slots.ctypes.data), "sfs_slots")
        groups = [self.lib.gph_engine_sfs_column_name(self.engine, NS + g).decode() for g in range(NG)]
        return slots, groups

    def sfs(self, reset=False):
        """the accumulators of this rank's Q selected loci as the device holds them: a dict of loci[Q] (global indices), samples,
        group (the selected loci a partial row sums), columns (the NS slot names), groups (the NG group names), slots (NS, 5) int32
        (group, kind, P, Q, k) and E (Q, NS) float64.  reset=True zeroes E afterwards and restarts the sample count"""
        NS, NG, G_, Q, S, _ = self._sfs_shape()
        slots, groups = self._sfs_tables()
        loci = self._selected(self.lib.gph_engine_sfs_selected, Q)
        acc = np.zeros((max(Q, 1), NS), dtype=np.float64)
        self._chk(self.lib.gph_engine_sfs_fetch_loci(self.engine, acc.ctypes.data, NS, int(bool(reset))), "sfs_fetch_loci")
        return dict(loci=loci, samples=S, group=G_, columns=self.sfs_columns(), groups=groups, slots=slots, E=acc[:Q].copy())

    def sfs_observed(self):
        """the data side, formed once at enable: a dict of loci[Q], obs (Q, NS), use (Q, NG), sites (Q,) uint32 and their totals over
        this rank's selected loci, obs_total (NS,), use_total (NG,), sites_total, uint64"""
        NS, NG, _, Q, _, _ = self._sfs_shape()
        if NS == 0:
            raise RuntimeError("gphocs_hip: sfs_observed: not enabled (GPH_ESTATE)")
        W = NS + NG + 1
        out = np.zeros((max(Q, 1), W), dtype=np.uint32)
        tot = np.zeros(W, dtype=np.uint64)
        self._chk(self.lib.gph_engine_sfs_fetch_observed(self.engine, out.ctypes.data, W, tot.ctypes.data), "sfs_fetch_observed")
        out = out[:Q]
        return dict(loci=self._selected(self.lib.gph_engine_sfs_selected, Q), obs=out[:, :NS].copy(), use=out[:, NS:NS + NG].copy(), sites=out[:, NS + NG].copy(),
                    obs_total=tot[:NS].copy(), use_total=tot[NS:NS + NG].copy(), sites_total=int(tot[NS + NG]))

    def sfs_rows(self):
        """(iterations, rows): the per-sample rows taken since the last call, a float64 (samples, NS) array -- per slot the expected
        number of sites of the class among the usable ones, over THIS rank's selected loci -- and their iterations; the device
        buffer is emptied"""
        NS, _, _, _, _, held = self._sfs_shape()
        if NS == 0:
            raise RuntimeError("gphocs_hip: sfs_rows: not enabled (GPH_ESTATE)")
        _, rows = self._fetch_rows(self.lib.gph_engine_sfs_fetch_rows, held, 1 + NS)
        return rows[:, 0].astype(np.int32), rows[:, 1:].copy()

    # ---- replicate genealogies simulated from the sampled parameters (gph_engine_simulate_*): simulated on the device
    def simulate_enable(self, seed, capacity, loci=None, with_sites=True, max_bytes=0):
        """per-locus accumulators of the replicate-against-sampled statistics for the selected loci (as enable_gene_trees; None:
        all loci of this rank), the latest sample's replicate records and a device buffer of `capacity` per-sample rows; capacity
        0 switches the feature off.  with_sites: the replicate alignment is drawn on the replicate genealogy as well.  The
        replicates are a pure function of (seed, locus, sample) and the model.  ValueError for a refused selection or a locus
        whose site statistics do not fit 32 bits, MemoryError when the buffers would exceed max_bytes (0: 1 GiB)"""
        sel = self._listed(None if loci is None else np.ascontiguousarray(loci, dtype=np.int64))
        self._enabled(self.lib.gph_engine_simulate_enable(self.engine, int(seed) & 0xffffffffffffffff, int(capacity), *sel, int(bool(with_sites)),
                                                          int(max_bytes)),
                      "simulate_enable", "the simulate accumulators, records and rows exceed", "the capacity, the selection or a locus")

    def simulate_sample(self, it):
        """one replicate genealogy of every selected locus under the current parameters, labelled iteration `it`; BufferError
        when the row buffer is full"""
        self._sample(self.lib.gph_engine_simulate_sample, "simulate row", "simulate_rows", int(it))

    def _simulate_shape(self):
        q, m, c, rc, rb, S, held = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32()
        self._chk(self.lib.gph_engine_simulate_shape(self.engine, C.byref(q), C.byref(m), C.byref(c), C.byref(rc), C.byref(rb), C.byref(S), C.byref(held)),
                  "simulate_shape")
        return q.value, m.value, c.value, rc.value, rb.value, S.value, held.value

    def simulate_columns(self, which=0):
        """which 0: the genealogy statistics, 1: the columns of a per-sample row, 2: the site statistics"""
        _, m, c, rc, _, _, _ = self._simulate_shape()
        return [self.lib.gph_engine_simulate_column_name(self.engine, which, k).decode() for k in range((m, rc, c)[which])]

    def simulate(self, reset=False):
        """the accumulators of this rank's Q selected loci as the device holds them: a dict of loci[Q] (global indices), samples,
        stats (the M names), acc (Q, M, 5) float64 -- gt, eq, sx, sy, sy2 --, failed[Q], and with sites site_stats (the C names),
        sites[Q], site_acc (Q, C, 5) -- obs, gt, eq, s1, s2.  reset=True zeroes them afterwards and restarts the sample count"""
        Q, M, Cn, _, _, S, _ = self._simulate_shape()
        if M == 0:
            raise RuntimeError("gphocs_hip: simulate: not enabled (GPH_ESTATE)")
        loci = self._selected(self.lib.gph_engine_simulate_selected, Q)
        names, snames = self.simulate_columns(0), self.simulate_columns(2)
        acc = np.zeros((max(Q, 1), 5 * M + 1), dtype=np.float64)
        sacc, sites = np.zeros((max(Q, 1), max(Cn, 1), 5), dtype=np.float64), np.zeros(max(Q, 1), dtype=np.int64)
        self._chk(self.lib.gph_engine_simulate_fetch_loci(self.engine, acc.ctypes.data, sacc.ctypes.data if Cn else None, sites.ctypes.data,
                                                          int(bool(reset))), "simulate_fetch_loci")
        return dict(loci=loci, samples=S, stats=names, acc=acc[:Q, :5 * M].reshape(Q, M, 5).copy(), failed=acc[:Q, 5 * M].copy(),
                    site_stats=snames, sites=sites[:Q].copy(), site_acc=sacc[:Q, :Cn].copy())

    def simulate_rows(self):
        """(iterations, rows, observed): the per-sample rows taken since the last call, a uint64 (samples, columns) array of the
        totals over THIS rank's selected loci (simulate_columns(1)), their iterations, and the data's site totals observed[C];
        the device buffer is emptied"""
        _, M, Cn, rc, _, _, held = self._simulate_shape()
        if M == 0:
            raise RuntimeError("gphocs_hip: simulate_rows: not enabled (GPH_ESTATE)")
        obs = np.zeros(max(Cn, 1), dtype=np.uint64)
        its, rows = self._fetch_rows(self.lib.gph_engine_simulate_fetch_rows, held, rc, np.uint64, with_iters=True, ld=False, extra=(obs.ctypes.data,))
        return its.copy(), rows.copy(), obs[:Cn]

    def simulate_records(self, raw=False):
        """the replicate genealogies of the latest sample, decoded as gene_trees() decodes a sample (arrays [Q, ...]); a failed
        replicate has root -1.  raw=True adds records: uint8 [Q, record_bytes]"""
        Q, M, _, _, rb, _, _ = self._simulate_shape()
        if M == 0:
            raise RuntimeError("gphocs_hip: simulate_records: not enabled (GPH_ESTATE)")
        N, Mg = 2 * self.pack.n - 1, GT_MAX_MIGS
        rec = np.zeros((max(Q, 1), max(rb, 1)), dtype=np.uint8)
        off = (C.c_int32 * GT_OFFSETS)()
        self._chk(self.lib.gph_engine_simulate_fetch_records(self.engine, rec.ctypes.data, off), "simulate_fetch_records")
        rec = np.ascontiguousarray(rec[:Q])
        out = dict(loci=self._selected(self.lib.gph_engine_simulate_selected, Q))
        shapes = dict(age=((Q, N), np.float64), father=((Q, N), np.int32), left=((Q, N), np.int32), right=((Q, N), np.int32),
                      npop=((Q, N), np.int32), root=((Q,), np.int32), num_migs=((Q,), np.int32), dataLnL=((Q,), np.float64),
                      genLnL=((Q,), np.float64), mig_branch=((Q, Mg), np.int32), mig_band=((Q, Mg), np.int32),
                      mig_spop=((Q, Mg), np.int32), mig_tpop=((Q, Mg), np.int32), mig_age=((Q, Mg), np.float64))
        for k, (shp, dt) in shapes.items():
            out[k] = np.zeros(shp, dtype=dt)
        if Q:
            self._chk(self.lib.gph_gene_trees_decode(rec.ctypes.data, Q, rb, off, N, *[out[k].ctypes.data for k in shapes]), "gene_trees_decode")
        if raw:
            out["records"] = rec
        return out

    def hbm_bytes(self):
        b = C.c_double()
        self._chk(self.lib.gph_engine_hbm_bytes(self.engine, C.byref(b)), "hbm_bytes")
        return b.value

    def close(self):
        if self.mcmc:
            self.lib.gph_mcmc_destroy(self.mcmc)
            self.mcmc = None
        if self.engine:
            self.lib.gph_engine_destroy(self.engine)
            self.engine = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MC3:
    """Metropolis-coupled chains on one device (gph_mc3_*): chain c runs on a copy of the pack seeded with seed + c and keeps
    betas[c]; at a swap point two neighbours exchange their states, so chains[0] stays the chain of betas[0]."""

    def __init__(self, pack, betas, swap_every=1, swap_seed=None, lib=None):
        import copy
        self.betas = [float(b) for b in betas]
        self.swap_every = int(swap_every)
        self.swap_seed = int(pack.seed + len(self.betas) if swap_seed is None else swap_seed)
        self.chains = []
        self.group = None
        for c in range(len(self.betas)):
            q = copy.copy(pack)
            q.seed = pack.seed + c
            self.chains.append(Sampler(q, lib=lib))
        self.lib = self.chains[0].lib if self.chains else (lib or load_library())

    def initialize(self):
        for s in self.chains:
            s.initialize()
        C_ = len(self.chains)
        hs = (C.c_void_p * max(C_, 1))(*[s.mcmc for s in self.chains])
        bs = (C.c_double * max(C_, 1))(*self.betas)
        g = C.c_void_p()
        Sampler._chk(self.lib.gph_mc3_create(hs, C_, bs, self.swap_every, self.swap_seed & 0xffffffff, C.byref(g)), "mc3_create")
        self.group = g

    def iteration(self, it):
        Sampler._chk(self.lib.gph_mc3_iteration(self.group, it), f"mc3 iteration {it}")

    def swap_counts(self):
        """(attempts, accepted), one entry per pair (c, c + 1)"""
        n = len(self.chains) - 1
        a, b = (C.c_int64 * n)(), (C.c_int64 * n)()
        Sampler._chk(self.lib.gph_mc3_swap_counts(self.group, a, b), "mc3_swap_counts")
        return list(a), list(b)

    def swap_log(self):
        """every swap decision so far, as dicts of the fields of gph_mc3_swap"""
        n = C.c_int64()
        Sampler._chk(self.lib.gph_mc3_swap_log(self.group, None, 0, C.byref(n)), "mc3_swap_log")
        buf = (GphMc3Swap * max(n.value, 1))()
        Sampler._chk(self.lib.gph_mc3_swap_log(self.group, buf, n.value, C.byref(n)), "mc3_swap_log")
        return [{f: getattr(buf[i], f) for f, _ in GphMc3Swap._fields_ if f != "pad"} for i in range(n.value)]

    def close(self):
        if self.group:
            self.lib.gph_mc3_destroy(self.group)
            self.group = None
        for s in self.chains:
            s.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
