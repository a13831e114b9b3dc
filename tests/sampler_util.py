"""Helpers the tests of the statistics samplers share (test_locus_summary.py, test_coal_stats.py, test_time_slices.py,
test_ancestry.py and their -m gpu twins): the launcher, golden cases copied into a scratch directory, names read from the
inputs themselves, and the host-emulation build the CPU tests load."""
import math
import os
import re
import shutil
import subprocess
import sys

from conftest import GOLDEN, REPO

sys.path.insert(0, os.path.join(REPO, "tests", "hostemu"))

EXE = os.path.join(REPO, "g-phocs_amd", "G-PhoCS-hip")
U = 2.0 ** -53


def hostemu_library():
    """(path, library) of the default host-emulation build; the body of the modules' `hostemu` fixtures"""
    import run_hostemu
    import gphocs_amd as G
    G.build()                       # the launcher executable (g++); the HIP libraries are not loaded here
    path = run_hostemu.build_hostemu()
    return path, G.load_library(path)


# launch shapes no golden has: a few loci from the benchmark's generator (g-phocs_amd/synth.py), the same data every time.
# name: (configuration there, loci)
SYNTHETIC = {"t136": (14, 2),       # 136 leaves: a gene-tree record of 290 units, one clade table a workgroup (three key words)
             "w139": (15, 2),       # 39 populations + 100 bands: the walkers of the time slices in more than one tile
             "a70": (1, 70)}        # 8 leaves, 70 loci: three groups of 32 loci in k_ancestry, migrations in few of them


def load_pack(name):
    """the pack of a case: golden `name`, or the synthetic data set of that name (SYNTHETIC)"""
    import gphocs_amd as G
    if name in SYNTHETIC:
        from gphocs_amd_pkg import synth
        config, loci = SYNTHETIC[name]
        return synth.make_synthetic_pack(G.Pack, config, loci, seqlen=200, samples_per_log=8)
    return G.Pack.load(os.path.join(GOLDEN, name + ".gpk"))


def _fmt(x):
    return "%.10g" % x


def _run(hostemu_path, cwd, args):
    """the launcher; hostemu_path None: the product libraries (the MI355X)"""
    env = dict(os.environ, GPHOCS_HIP_LIB=hostemu_path) if hostemu_path else dict(os.environ)
    r = subprocess.run([EXE] + args, cwd=cwd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r


def _copy_case(name, dst, ctl_text=None):
    os.makedirs(dst, exist_ok=True)
    for ext in (".ctl", ".seq"):
        shutil.copy(os.path.join(GOLDEN, name + ext), dst)
    if ctl_text is not None:
        open(os.path.join(dst, name + ".ctl"), "w").write(ctl_text)


def _pop_names(ctl_path):
    """population names in model order (current populations first, then ancestral), from the control file itself"""
    txt = open(ctl_path).read()
    cur = re.search(r"CURRENT-POPS-START(.*?)CURRENT-POPS-END", txt, re.S).group(1)
    anc = re.search(r"ANCESTRAL-POPS-START(.*?)ANCESTRAL-POPS-END", txt, re.S).group(1)
    return re.findall(r"^\s*name\s+(\S+)", cur, re.M) + re.findall(r"^\s*name\s+(\S+)", anc, re.M)


def _locus_names(seq_path):
    tok = open(seq_path).read().split("\n")
    names, i = [], 0
    L = int(tok[0].split()[0])
    i = 1
    while len(names) < L:
        t = tok[i].split()
        i += 1
        if len(t) == 3:
            names.append(t[0])
            i += int(t[1])
    return names


def _data_lines(trace):
    return open(trace).read().splitlines()[1:]


def within_bound(got, want, T):
    """relative difference <= (2T + 4) * 2^-53"""
    if got == want:
        return True, 0.0
    rel = abs(got - want) / abs(want) if want != 0.0 else math.inf
    return rel <= (2 * T + 4) * U, rel


def printed_names(sample_names):
    """the second haploid of a diploid has no name: the previous sample's, NA without one (GPhoCS.c:942-953)"""
    out = []
    for i, nm in enumerate(sample_names):
        if not nm:
            nm = sample_names[i - 1] if i > 0 and sample_names[i - 1] else "NA"
        out.append(nm)
    return out


def read_outputs(d, prefix):
    return {f[len(prefix) + 1:]: open(os.path.join(d, f)).read() for f in sorted(os.listdir(d)) if f.startswith(prefix + ".")}


RANK_WORKER = r'''
import os, sys
sys.path.insert(0, %(repo)r)
import gphocs_amd as G
rank, world = int(sys.argv[1]), int(sys.argv[2])
lib = G.load_library(%(lib)r) if %(lib)r else G.load_library(dims=%(dims)r)
comm = lib.gph_comm_create_shm(%(name)r.encode(), rank, world)
assert comm
os.chdir(%(cwd)r)
rc = G.run_control_file(lib, %(ctl)r, comm=comm, **%(options)r)
sys.stdout.flush()
if rc == 0:
    lib.gph_comm_destroy(comm)
os._exit(1 if rc else 0)
'''


def run_ranks(lib_path, name, ranks, d, **options):
    """`ranks` processes over a shared-memory communicator, each the program's own loop on golden `name` in directory d with
    the outputs that `options` (those of gphocs_amd.run_control_file) switch on: their parts stay.  The pack of the golden."""
    import gphocs_amd as G
    pk = G.Pack.load(os.path.join(GOLDEN, name + ".gpk"))
    _copy_case(name, d)
    script = d / "w.py"
    script.write_text(RANK_WORKER % dict(repo=REPO, lib=lib_path, dims=(pk.n, pk.K, pk.B), name=f"/gphocs-{os.getpid()}-{d.name}-{name}-{ranks}",
                                         cwd=str(d), ctl=name + ".ctl", options=options))
    procs = [subprocess.Popen([sys.executable, str(script), str(r), str(ranks)], stdout=subprocess.DEVNULL) for r in range(ranks)]
    for p in procs:
        assert p.wait(timeout=600) == 0
    return pk
