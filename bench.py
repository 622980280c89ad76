#!/usr/bin/env python3
"""
bench.py -- the reference's headline metric on MI355X: d_msm G1 scalar-muls/s (+ d_sumcheck Fr
field-ops/s) at 2^20 shares (BASELINE.json configs[1]/[2]), 1/2/4/8 GPUs.

A "step" = one party's d_msm on 2^20 packed BLS12-381 G1 shares: the local `G::msm`
(dist-primitive/src/dmsm.rs:19-24) on HBM-resident bases and scalars, followed -- when more than one
rank runs -- by its exchange step over RCCL/xGMI:
   8 ranks   the l = 1, 8-party d_msm end to end (zk_d_msm: all-gather of the 144-byte results +
             the public unpack2/pack map, dmsm.rs:29-40);
   2, 4      one MSM over N x 2^20 points cut into contiguous chunks, one per GPU:
             all-gather of the N partial points + local additions.
One process per GPU, rank = party; per-GPU work is fixed => "scaling": "weak".

    python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps and prints the line: the headline `value` with the phase split and the
roofline of the timed steps themselves.  --dump-outputs DIR then also writes the result of the last timed step to DIR (inputs
are seeded: the same arguments give the same inputs, so two builds can be compared output for output).  --full adds every
other leg listed below; it is what the tests, the profile collection and the runbooks use.

N > 1 runs one process per GPU over torch.distributed (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from the environment when a
launcher provides them).  Started WITHOUT a launcher, `python bench.py --gpus N` launches itself: it re-executes under
`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1` (default), or -- with --party-threads --
stays ONE process holding a ctx per GPU, zk_comm_init_all and one host thread per party (the reference's own model,
mpc-net/src/multi.rs:330-352).  With fewer than N GPUs it prints a JSON line carrying "error" and exits non-zero.
ZK_BENCH_BACKEND=gloo (processes) / =local (party threads) exercise the N > 1 code path on a box with fewer GPUs than ranks
(ranks then share GPUs round-robin; the exchanges travel through the host): functional records, not scaling figures.

Rank 0 prints ONE JSON line.  Besides the contract fields it carries (the legs after msm_phase_ms / roofline with --full only)
  roofline       dominant kernel (bucket accumulation), HIP-event timed inside the library on its own stream
  strong         STRONG scaling of one primitive over the N ranks (zkhip/sharding.py): one 2^20 MSM, one
                 2^24 MSM, one 2^24 product sumcheck -- total work fixed, split N ways
  sumcheck       the sumcheck family at 2^20 / 2^24 / 2^26 against the HBM roofline (N = 1)
  e2e            collaborative HyperPlonk l = 1, n = 20: leader mode at N = 1, the real 8-party run at N = 8;
                 every run verifies its own transcripts (zkhip.verify) -- the figure is not reported otherwise
  cpu_baseline   the C port of the reference's single-threaded path on this box's host cores (N = 1 only)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "scalable-collaborative-zksnark_amd"))
# multi-process GPU work (RCCL across ranks) needs dmabuf IPC on this driver stack; the launcher normally exports it already
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np  # noqa: E402

LOG2_N = 20
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec
MAD_PEAK = 34.3e12  # measured v_mad_u64_u32 issue rate, lane-ops/s, whole chip (profiles/r01_ubench_int_alu.txt)
MADS_PER_MADD = 6 * 338 + 2 * 260 + 507  # XYZZ mixed addition on 13x30-bit limbs: 6 mul + 2 sqr + 1 fused two-product mul (csrc/curve30.cuh)
FR_MUL_PEAK = 133.0e9  # measured Fr Montgomery mul/s (same file)


def transcript_sha256(res) -> str:
    """SHA-256 over a dhyperplonk result in the reference's order (raw limbs): what host/examples/hyperplonk.cpp --digest prints"""
    import hashlib

    import numpy as np

    ((gp, gc), (wp, wc, wo)) = res
    b = lambda *arrs: b"".join(np.ascontiguousarray(a, dtype=np.uint64).tobytes() for a in arrs)
    return hashlib.sha256(b(*gp) + b"".join(b(c, v, prf) for c, (v, prf) in gc) + b(*wp) + b(*wc) + b"".join(b(v, prf) for v, prf in wo)).hexdigest()


def cpp_host_e2e(n: int, reps: int = 4, want_digest: str = None, check: bool = False, serial_rep: bool = False, timeout: int = 900, mode: str = "leader",
                 share_gpus: bool = False, env: dict = None, which: str = "dhyperplonk", arena_plan: str = None):
    """
    The same proof driven by the COMPILED host (scalable-collaborative-zksnark_amd/host: zkhost/hyperplonk.hpp, the C++ mirror of the
    reference's Rust crates above the C ABI) in its own process: leader mode, the SplitMix64 parameter set of the e2e leg (seed 100,
    challenges 4242), best of `reps`.  Self-checks: (want_digest) its transcript digest must equal the digest of the Python driver's
    transcript on the same parameter set -- the run the anchored check of the e2e leg has just verified; (check) the host's own
    anchored verifier (`--check`, zkhost/verify.hpp: no Python, no oracle in the loop) must print `ok`.  A figure that fails either
    is withdrawn.  mode = "rccl": ONE process, party p on GPU p, exchanges over RCCL (zk_comm_init_all) -- the 8-GPU form of the same
    binary; every party must print its own `ok` (share_gpus: only the test double of librccl accepts several ranks per device).
    """
    import subprocess

    exe = os.path.join(ROOT, "scalable-collaborative-zksnark_amd", "host", "bin", "hyperplonk")
    if not os.path.exists(exe):
        return {"error": "host/bin/hyperplonk is not built (__graft_entry__.build())"}
    try:
        cmd = [exe, "--l", "1", "--n", str(n), "--reps", str(reps), "--digest"] + (["--check"] if check else []) + (["--serial-rep"] if serial_rep else [])
        cmd += (["--mode", mode] if mode != "leader" else []) + (["--share-gpus"] if share_gpus else []) + (["--which", which] if which != "dhyperplonk" else [])
        cmd += ["--arena-plan", arena_plan] if arena_plan else []  # (imported after the setup when the file exists, written after the repetitions)
        TOT = {"dhyperplonk": "Distributed HyperPlonk", "data-parallel": "Distributed HyperPlonk", "dpermcheck": "Distributed Permcheck", "cpermcheck": "Collaborative Permcheck"}[which]
        parties = 1 if mode == "leader" else 8
        t0 = time.perf_counter()
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)
        wall = time.perf_counter() - t0
        if r.returncode != 0:
            return {"error": f"rc {r.returncode}: {(r.stdout[-400:] + r.stderr[-300:])}"}
        runs, comm, digests, serial, checks, setup, plan_note = [], None, set(), {}, [], None, None
        for line in r.stdout.splitlines():
            w = line.split()
            if line.startswith("arena plan "):
                plan_note = line
            elif line.startswith("rep "):
                runs.append({})
                setup = float(w[3])
            elif line.startswith("  End(serial):"):
                serial[" ".join(w[1:-2])] = float(w[-2])
            elif line.startswith("  End:") and runs:
                runs[-1][" ".join(w[1:-2])] = float(w[-2])
            elif line.startswith("Comm:"):
                comm = line[len("Comm: "):]
            elif line.startswith("transcript sha256"):
                digests.add(w[-1])
            elif line.startswith("check: party "):
                checks.append(line[len("check: "):])
        best = min(runs, key=lambda t: t.get(TOT, 1e9))
        out = {"timers_s": best, "first_proof_s": runs[0].get(TOT), "comm_per_proof": comm, "reps": reps, "transcript_sha256": sorted(digests),
               "setup_s": setup, "process_wall_s": wall,
               "timers_note": "'Commit' / 'Wire identity' / 'Open' of timers_s are OVERLAPPED sections (a step's MSM pass is started asynchronously and collected later; the kernel phase of "
                              "the Open step runs inside 'Wire identity'): they are not the reference's phases of the same name, only 'Distributed HyperPlonk' is comparable. "
                              "timers_s_serial_steps (when present) runs every pass to completion inside its own step",
               "first_proof_note": "the first proof of a process also allocates the library's MSM arenas and job lanes (sized by demand); later proofs reuse them; a process that imports the arena plan of an earlier one (zk_arena_plan_import) skips that: second_process_with_arena_plan",
               "what": "the same call sequence on the same parameter set from the compiled C++ host (zkhost/hyperplonk.hpp) in its own process, "
                       + ("leader mode" if mode == "leader" else f"--mode {mode}: 8 parties = 8 host threads of one process, party p on GPU p, exchanges over RCCL")}
        if arena_plan:
            out["arena_plan"] = plan_note or "none found: this run sized its arenas on demand and wrote the plan"
        if mode != "leader":
            out["stderr_tail"] = r.stderr[-300:]
        if which not in ("dhyperplonk", "data-parallel"):
            out.pop("timers_note")  # (one section, no overlapped steps)
            out["what"] = out["what"].replace("the same call sequence", f"`--which {which}`")
        if serial:
            out["timers_s_serial_steps"] = serial
        if check:
            ok = len(checks) == parties and all(" ok -- anchored" in c and "flipped limb rejected" in c for c in checks) and len(digests) == 1
            out["self_check"] = (sorted(checks)[0] if parties == 1 else sorted(checks)) if checks else "no check line"
            out["self_check_ok"] = ok
            out["transcript_check_kind"] = "anchored by the compiled host itself (hyperplonk --check): every chain pinned at both ends by independent kernels, c_ tails and sampled commits / opens recomputed, flipped limb rejected"
            if not ok:
                out["timers_s"] = None
        if want_digest is not None:
            out["transcript_equals_python_host"] = digests == {want_digest}
            if digests != {want_digest}:
                out["timers_s"] = None  # an unverified figure is not a figure
        return out
    except Exception as ex:
        return {"error": repr(ex)}


def pmc_traffic(kernel: str, pick: str = "most_dispatches"):
    """
    Memory-side bytes per launch of `kernel` from the newest committed rocprofv3 PMC passes of this command
    (profiles/*pmc_hbm_traffic.csv: FETCH_SIZE and WRITE_SIZE, KB per dispatch, separate passes; FETCH_SIZE
    doubled as MI355X_MICROARCH.md prescribes for gfx950, calibrated in profiles/r01_fetch_calibration.txt).
    Returns (bytes, file name): the counters cannot be read inside an un-profiled run, so the source is named.
    """
    import csv
    import glob

    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*pmc_hbm_traffic.csv")))
    if not files:
        return None, None
    best = {}  # counter -> (rank key, KB): the launch geometry with the most dispatches is the headline loop's, the largest grid the 2^24 leg's
    for row in csv.reader(open(files[-1])):
        if len(row) >= 5 and kernel in row[1] and row[0] in ("FETCH_SIZE", "WRITE_SIZE"):
            disp, kb = int(row[-2]), float(row[-1])
            key = disp if pick == "most_dispatches" else int(row[-3])
            if row[0] not in best or key > best[row[0]][0]:
                best[row[0]] = (key, kb)
    tot = sum(kb * 1024.0 * (2.0 if c == "FETCH_SIZE" else 1.0) for c, (_, kb) in best.items())
    return (tot or None), os.path.relpath(files[-1], ROOT)


def sort_phase_traffic():
    """FETCH_SIZE x 2 + WRITE_SIZE over the kernels of the round-6 sort phase at 2^24 points, from the newest committed profiles/*sort_phase_pmc.csv
    (its first block = the round-6 kernels; the block behind the `# r05` line = the round-5 kernels, not counted)"""
    import csv
    import glob

    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*sort_phase_pmc.csv")))
    if not files:
        return None, None
    tot = 0.0
    for line in open(files[-1]):
        if line.startswith("# r05"):
            break
        row = next(csv.reader([line]))
        if len(row) >= 5 and row[0] in ("FETCH_SIZE", "WRITE_SIZE"):
            tot += float(row[-1]) * 1024.0 * (2.0 if row[0] == "FETCH_SIZE" else 1.0)
    return (tot or None), os.path.relpath(files[-1], ROOT)


METRIC = "G1 scalar-muls/sec (d_msm) + Fr field-ops/sec (d_sumcheck), 2^20 shares, 1/2/4/8 GPU"
MAD_PEAK_ARCH = 256 * 128 * 2.4e9 / 2  # architectural ceiling: 256 CUs x 128 lanes/clk x 2.4 GHz, v_mad_u64_u32 at half rate = 39.3 T/s


def error_line(n_gpus: int, msg: str, **kw) -> str:
    """the line printed instead of a measurement when the run cannot take place (the driver sees WHY, never a traceback)"""
    return json.dumps(dict({"metric": METRIC, "value": None, "unit": "G1 scalar-muls/s", "n_gpus": n_gpus, "error": msg}, **kw))


class ProcGroup:
    """the ranks of this run = processes of torch.distributed (world 1: no process group at all)"""

    def __init__(self, rank, world, backend, dev):
        self.rank, self.world, self.backend, self.dev = rank, world, backend, dev
        self.kind = "one process per GPU (torch.distributed)" if world > 1 else "single process"

    def barrier(self):
        if self.world > 1:
            import torch.distributed as dist

            dist.barrier()

    def allmax(self, x: float) -> float:
        if self.world == 1:
            return x
        import torch
        import torch.distributed as dist

        t = torch.tensor([x], device=self.dev if self.backend == "nccl" else "cpu", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    def all_gather_obj(self, obj) -> list:
        if self.world == 1:
            return [obj]
        import torch.distributed as dist

        out = [None] * self.world
        dist.all_gather_object(out, obj)
        return out

    def finish(self):
        if self.world > 1:
            import torch.distributed as dist

            dist.barrier()
            dist.destroy_process_group()


class ThreadGroup:
    """the ranks of this run = party threads of ONE process (mpc-net/src/multi.rs:330-352), a ctx per party"""

    kind = "one process, one host thread per party (zk_comm_init_all)"

    class Hub:
        def __init__(self, n):
            import threading

            self.n, self.slots, self.bar = n, [None] * n, threading.Barrier(n)

    def __init__(self, hub, rank, backend):
        self.hub, self.rank, self.world, self.backend, self.dev = hub, rank, hub.n, backend, None

    def barrier(self):
        self.hub.bar.wait()

    def all_gather_obj(self, obj) -> list:
        self.hub.slots[self.rank] = obj
        self.hub.bar.wait()
        out = list(self.hub.slots)
        self.hub.bar.wait()
        return out

    def allmax(self, x: float) -> float:
        return max(self.all_gather_obj(x))

    def finish(self):
        self.hub.bar.wait()


def timed(fn, reps, barrier):
    barrier()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    barrier()
    return (time.perf_counter() - t0) / reps


def device_table(ctx, log2n: int, seed: int):
    """2^log2n pseudo-random Fr in HBM without a host array of that size: a 2^20 random block, every further
    block an affine image alpha_k * block + beta_k (the kernels' timing does not depend on the values)"""
    from zkhip.field import random_fr

    n, blk = 1 << log2n, 1 << min(log2n, 20)
    base = ctx.to_device(random_fr(blk, seed))
    if n == blk:
        return base
    out = ctx.alloc(32 * n)
    ab = random_fr(2 * (n // blk), seed + 1)
    for k in range(n // blk):
        ctx.fr_axpb(None, base, ab[2 * k], ab[2 * k + 1], blk, out=out.at(32 * blk * k))
    return out


def _at_least(lo: int):
    def parse(s: str) -> int:
        v = int(s)
        if v < lo:
            raise argparse.ArgumentTypeError(f"must be >= {lo}, got {v}")
        return v

    return parse


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=_at_least(1), default=50, help="timed steps (ms_per_step = their wall time / steps)")
    ap.add_argument("--warmup", type=_at_least(0), default=3)
    ap.add_argument("--full", action="store_true",
                    help="run every leg beside the headline (table-less and pipelined MSM, strong scaling, sumcheck family, end-to-end proofs, G2, "
                         "CPU baseline); off: set up, warm up, time the steps, print the line")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write the last step's MSM result (normalised Jacobian, 18 uint64 limbs) as DIR/msm_g1_result.npy "
                         "(DIR/msm_g1_result_rank<r>.npy per rank when N > 1): float64, the limbs as little-endian 32-bit words, shape [..., 36]")
    ap.add_argument("--log2n", type=int, default=LOG2_N)
    ap.add_argument("--cpu-log2n", type=int, default=20, help="size of the bounded CPU-baseline MSM sample")
    ap.add_argument("--cpu-e2e-n", type=int, default=13, help="log2 constraints of the CPU end-to-end sample")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-precompute", action="store_true", help="time the MSM without the SRS window table (zk_srs_precompute)")
    ap.add_argument("--table-rec", type=int, default=0, choices=(0, 96, 128),
                    help="bytes per record of the G1 window tables of the MSM legs: 0 = the library's own choice (zk_srs_precompute: 128-B records -- one per cache line -- while the table leaves >= 60 %% of the device free, "
                         "packed 96-B records otherwise; the hosts' parameter sets apply the same rule per level), 96 / 128 = forced (A/B)")
    ap.add_argument("--no-extra", action="store_true", help="headline + roofline only (profiling runs)")
    ap.add_argument("--no-e2e", action="store_true", help="skip the end-to-end leg (counter-collection runs)")
    ap.add_argument("--no-e2e-n24", action="store_true", help="skip the n = 24 end-to-end leg (C++ host, ~25 s)")
    ap.add_argument("--big", type=int, default=24, help="log2 size of the large strong-scaling / sumcheck legs")
    ap.add_argument("--e2e-n", type=int, default=20, help="log2 constraints of the end-to-end leg (BASELINE configs[3]: 20)")
    ap.add_argument("--party-threads", action="store_true",
                    help="N > 1 without a launcher: ONE process, a ctx per GPU, zk_comm_init_all, one host thread per party (default: re-exec under torch.distributed.run)")
    return ap.parse_args()


def _free_port() -> int:
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def main():
    args = parse_args()
    N = args.gpus
    if N < 1 or (N & (N - 1)):
        print(error_line(N, f"--gpus {N}: the party / shard count must be a power of two (1, 2, 4, 8)"), flush=True)
        sys.exit(2)
    env_world = os.environ.get("WORLD_SIZE")
    backend = os.environ.get("ZK_BENCH_BACKEND", "nccl")  # nccl (= RCCL; real runs) | gloo (processes) / local (party threads): functional runs
    if env_world is not None and int(env_world) != N:
        print(error_line(N, f"--gpus {N} but the launcher set WORLD_SIZE={env_world}"), flush=True)
        sys.exit(2)
    import torch

    found = torch.cuda.device_count()
    if found == 0:
        print(error_line(N, "no GPU visible: zkhip has no CPU fallback", gpus_found=0), flush=True)
        sys.exit(3)
    shares = backend in ("gloo", "local")  # functional runs: ranks may share GPUs, exchanges staged through the host
    if N > found and not shares:
        print(error_line(N, f"needs {N} GPUs, found {found}", gpus_found=found), flush=True)
        sys.exit(3)
    if N > 1 and env_world is None:  # started without a launcher
        if args.party_threads:
            return run_party_threads(args, found, "local" if shares else "rccl")
        import subprocess

        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={N}", "--master-addr", "127.0.0.1",
               "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.run(cmd, env=dict(os.environ, OMP_NUM_THREADS=os.environ.get("OMP_NUM_THREADS", "4"))).returncode)

    world = N
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    gpu = local_rank % found
    torch.cuda.set_device(gpu)
    dev = torch.device("cuda", gpu)
    if world > 1:
        import torch.distributed as dist

        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
    import zkhip

    ctx = zkhip.Ctx(gpu)  # raises if libzkhip.so / the GPU is missing (no fallback)
    net = None
    if world > 1:
        from zkhip.net import RcclNet, TorchDistNet

        # the C-ABI communicator (RCCL inside the ctx); torch.distributed only hands the RCCL id around
        if backend == "nccl":
            try:
                net = RcclNet.from_torch_dist(ctx)
            except Exception as ex:  # the in-ctx communicator could not be set up: torch.distributed's RCCL carries the exchanges
                print(f"rank {rank}: RcclNet unavailable ({ex!r}), falling back to TorchDistNet", file=sys.stderr)
                net = TorchDistNet(device=dev)
        else:
            net = TorchDistNet()
    run_rank(args, ProcGroup(rank, world, backend, dev), gpu, ctx, net)


def run_party_threads(args, found: int, backend: str):
    """N parties = N host threads of this process, a ctx each; RCCL communicators from zk_comm_init_all (backend "rccl"), or --
    on a box with fewer GPUs than parties -- the thread net of the tests (backend "local": a functional run)"""
    import threading

    import zkhip
    from zkhip.net import LocalTestNet, RcclNet, _LocalHub

    N = args.gpus
    ctxs = [zkhip.Ctx(p % found) for p in range(N)]
    if backend == "rccl":
        nets = RcclNet.from_init_all(ctxs)
    else:
        lh = _LocalHub(N)
        nets = [LocalTestNet(lh, p) for p in range(N)]
    hub = ThreadGroup.Hub(N)
    errors = []

    def party(p):
        try:
            import torch

            torch.cuda.set_device(p % found)
            run_rank(args, ThreadGroup(hub, p, backend), p % found, ctxs[p], nets[p])
        except BaseException as e:  # noqa: BLE001
            errors.append((p, e))
            hub.bar.abort()
            if hasattr(nets[p], "hub"):
                nets[p].hub.barrier.abort()

    ths = [threading.Thread(target=party, args=(p,)) for p in range(N)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    if errors:
        print(error_line(N, "party thread %d failed: %r" % errors[0]), flush=True)
        sys.exit(1)


def run_rank(args, grp, gpu: int, ctx, net):
    import torch

    import zkhip
    from zkhip.field import int_to_limbs, random_fr

    world, rank, backend = grp.world, grp.rank, grp.backend
    extra_legs = args.full and not args.no_extra  # a plain run does only what the headline needs
    n = 1 << args.log2n
    pp = None
    if world == 8:
        from zkhip.pss import PackedSharingParams

        pp = PackedSharingParams(1)

    def barrier():
        ctx.sync()
        torch.cuda.synchronize()
        grp.barrier()
        torch.cuda.synchronize()

    # ---- synthetic inputs, resident in HBM before the timed region ----
    seed = 0x5CA1AB1E + 1000 * 2 + rank
    srs = ctx.srs_generate(0x1234567 + rank, 0x89ABCDE + 7 * rank, n)  # P_i = (k0 + i k1) G, built on the device
    scal_np = random_fr(n, seed)
    scalars = ctx.to_device(scal_np)
    chal = random_fr(32, seed + 3)
    ones = np.tile(int_to_limbs(1, 4), (max(world, 1), 1))

    from zkhip import sharding as sh

    def step():
        if world == 1:
            return ctx.msm_g1(srs, scalars, n)
        if pp is not None:  # the full 8-party d_msm (zk_d_msm when the communicator lives in the ctx)
            from zkhip.dist_primitive import d_msm

            return d_msm(ctx, [srs], [scalars], [n], pp, net)
        return sh.sharded_msm(ctx, srs, scalars, n, net)  # one MSM of world * 2^20 points, a chunk per GPU

    # The SRS is fixed for the life of a prover (PolynomialCommitmentCub::new, dpoly_comm.rs:37-67): like uploading it, the
    # window table 2^{o_w} P_i (zk_srs_precompute) is built once, outside the timed region.  With it every digit of a scalar
    # lands in ONE bucket set, so the window can be 19 bits wide at 2^20 points: 14 bucket additions per scalar instead of
    # 16, one bucket reduction instead of 8.  The table-less path is timed first (a few steps) and reported beside it (--full).
    default_path = None
    if not args.no_precompute:
        if extra_legs:  # (plain and profiling runs time the headline geometry only)
            for _ in range(2):
                step()
            ph0 = np.zeros(6)
            barrier()
            t0 = time.perf_counter()
            for _ in range(10):
                step()
                ph0 += ctx.msm_last_timing()
            barrier()
            dt0 = (time.perf_counter() - t0) / 10
            c0 = ctx.lib.zk_msm_window(n)
            default_path = {"scalar_muls_per_s": world * n / dt0, "ms_per_step": dt0 * 1e3, "steps": 10, "pippenger_window_bits": c0, "windows": (129 + c0 - 1) // c0,
                            "k_accum_tiles_ms": float(ph0[1]) / 10, "note": "no window table: endomorphism split, 2n entries per window, one bucket set per window"}
        # the table layout is the library's own choice (zk_srs_precompute: 128-B records while the device has the room, packed otherwise) --
        # the rule the hosts' parameter sets apply per level, so the MSM legs and the proof legs of this line run the same layout policy;
        # config.srs_window_table.record_bytes says what was built
        t0 = time.perf_counter()
        srs.precompute(0, record_bytes=args.table_rec)
        ctx.sync()
        precompute_s = time.perf_counter() - t0
    for _ in range(args.warmup):
        step()
    phase = np.zeros(6)
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        last = step()
        phase += ctx.msm_last_timing()
    barrier()
    dt = grp.allmax(time.perf_counter() - t0)
    phase /= args.steps
    if args.dump_outputs:
        # what a caller of the step receives (uint64 limbs), as float64 of its exact 32-bit words
        os.makedirs(args.dump_outputs, exist_ok=True)
        words = np.ascontiguousarray(np.asarray(last, dtype="<u8")).view("<u4").astype(np.float64)
        np.save(os.path.join(args.dump_outputs, "msm_g1_result.npy" if world == 1 else f"msm_g1_result_rank{rank}.npy"), words)
    # who ran: one entry per rank (the driver can see that RCCL really had N ranks on N distinct devices)
    rccl_ranks = int(ctx.comm_size) if (net is not None and type(net).__name__ == "RcclNet") else 0
    who = grp.all_gather_obj({"rank": rank, "gpu": gpu, "name": torch.cuda.get_device_name(gpu), "pid": os.getpid(), "zk_comm_size": rccl_ranks})

    # the same K steps with up to three of them in flight (zk_msm_g1_batch_async / zk_msm_wait: the latency-bound tail of one MSM --
    # fix-up, 18 reduction passes, host chain -- runs beside the accumulation of the next two).  Every result is collected inside
    # the timed region.  Reported beside `value`, which stays the one-call-at-a-time figure.
    pipelined = None
    if world == 1 and extra_legs:
        try:
            def run_pipelined(k, depth=3):
                jobs = []
                for _ in range(k):
                    jobs.append(ctx.msm_g1_batch_async([srs], [scalars], [n]))
                    if len(jobs) >= depth:
                        jobs.pop(0).wait()
                for j in jobs:
                    j.wait()

            run_pipelined(9)  # (the job lanes allocate their arenas on first use)
            barrier()
            t0 = time.perf_counter()
            run_pipelined(args.steps)
            barrier()
            dtp = time.perf_counter() - t0
            pipelined = {"steps": args.steps, "in_flight": 3, "ms_per_step": dtp / args.steps * 1e3, "scalar_muls_per_s": n * args.steps / dtp,
                         "note": "same MSM, same results, three calls in flight on the ctx's job lanes; `value` above is the blocking one-call-at-a-time figure"}
        except Exception as ex:
            pipelined = {"error": repr(ex)}

    # ---- the contract line is complete at this point; everything below only ADDS legs to it.  A watchdog makes
    # sure the line is printed even if a later leg hangs (a collective of an untested multi-GPU path waiting for a
    # rank that failed): past the deadline rank 0 prints what it has and every rank leaves. ----
    import threading

    out = None
    if rank == 0:
        value = world * n * args.steps / dt
        accum_ms = float(phase[1])
        alg_bytes = 128.0 * n  # 96-B affine point + 32-B scalar per scalar-mul, read once
        achieved = alg_bytes / (accum_ms * 1e-3) / 1e9 if accum_ms > 0 else 0.0
        tc = srs.table_window
        if tc:
            c, windows, per_window = tc, (256 + tc - 1) // tc, n  # table mode: ceil(256 / c) digits per scalar, one bucket set
        else:
            c = ctx.lib.zk_msm_window(n)
            windows, per_window = (129 + c - 1) // c, 2 * n  # scalars are split into two 128-bit halves (k = k1 + k2*lambda): 2n entries per window
        madds = float(per_window) * windows  # one XYZZ mixed addition per entry per window
        traffic, traffic_src = pmc_traffic("k_accum_tiles") if args.log2n == 20 else (None, None)
        out = {
            "metric": METRIC,
            "value": value,
            "unit": "G1 scalar-muls/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u32",
            "data": "synthetic",
            "config": {
                "workload": f"d_msm on 2^{args.log2n} packed BLS12-381 G1 shares per party (BASELINE.json configs[1]), l=1",
                "points_per_party": n,
                "parties": world,
                "exchange": "none" if world == 1 else ("zk_d_msm: RCCL all-gather of the 144-B results + PSS unpack2/pack map (dmsm.rs:29-40)" if world == 8
                                                      else "one MSM over N x 2^20 points, a contiguous chunk per GPU: RCCL all-gather of N partial points + additions"),
                "pippenger_window_bits": c,
                "windows": windows,
                "entries_per_window": per_window,
                "srs_window_table": ({"window_bits": tc, "copies": windows, "bytes": windows * ((n + 3) & ~3) * srs.table_record, "record_bytes": srs.table_record, "record_policy": ("library default: by free memory" if not args.table_rec else "forced by --table-rec"),
                                      "record_note": "128 = one G1 record per 128-B line, 96 = packed; zk_srs_precompute and the hosts' parameter sets (per level) choose 128 while the table leaves >= 60 % of the device free", "build_s": precompute_s,
                                      "built": "once per SRS level, outside the timed region (zk_srs_precompute)"} if tc else None),
            },
            "rccl_ranks": rccl_ranks,  # = zk_comm_size of the in-ctx communicator (0: no RCCL communicator in this run)
            "exchange_backend": ("none (one GPU)" if world == 1 else {"RcclNet": "rccl: zk_comm inside the ctx (zk_d_msm / zk_allgather / zk_alltoall on HBM buffers over xGMI)",
                                                                     "TorchDistNet": f"torch.distributed {backend} (host-staged numpy payloads)",
                                                                     "LocalTestNet": "party threads exchanging through host memory (functional run, no wire)"}.get(type(net).__name__, type(net).__name__)),
            "ranks": {"model": grp.kind, "devices": who, "distinct_gpus": len({w["gpu"] for w in who})},
            "msm_without_window_table": default_path,
            "msm_three_calls_in_flight": pipelined,
            "msm_phase_ms": {"digits_sort": float(phase[0]), "k_accum_tiles": accum_ms, "fixup": float(phase[2]), "bucket_reduce": float(phase[3]), "host_combine": float(phase[4])},
            # The dominant kernel is bound by the 32-bit integer multiplier ("not HBM and not MFMA"): the roofline
            # object prices it against the MEASURED v_mad_u64_u32 issue rate of the chip; the HBM figure the north star asks for
            # (algorithmic 128 B per scalar-mul over the kernel's HIP-event time, against 8 TB/s) sits beside it under "hbm".
            "roofline": {
                "kernel": "zk::k_accum_tiles (bucket accumulation)",
                "bound": "int_alu",
                "achieved": (madds * MADS_PER_MADD / (accum_ms * 1e-3) / 1e12) if accum_ms > 0 else 0.0,
                "peak": MAD_PEAK / 1e12,
                "unit": "T v_mad_u64_u32/s",
                "frac": (madds * MADS_PER_MADD / (accum_ms * 1e-3) / MAD_PEAK) if accum_ms > 0 else 0.0,
                "traffic": traffic,
                "traffic_source": traffic_src,
                "mads_per_mixed_addition": MADS_PER_MADD,
                "mixed_additions_per_launch": madds,
                "kernel_ms": accum_ms,
                "peak_source": "profiles/r01_ubench_int_alu.txt (v_mad_u64_u32 issue rate measured on this chip, carry to SGPR)",
                "peak_architectural": MAD_PEAK_ARCH / 1e12,
                "frac_of_architectural": (madds * MADS_PER_MADD / (accum_ms * 1e-3) / MAD_PEAK_ARCH) if accum_ms > 0 else 0.0,
                "peak_architectural_note": "256 CU x 128 lanes/clk x 2.4 GHz / 2 (v_mad_u64_u32 issues at half rate); the chip clocks down to ~1.85 GHz under multiply-dense code, which is the gap to the measured peak",
                "counters": "profiles/r05z_accum_valu_counters.csv (SQ_INSTS_VALU, SQ_ACTIVE_INST_VALU, SQ_BUSY_CYCLES, SQ_WAVE_CYCLES of this kernel: 4 410 VALU instructions per mixed addition, 3 055 of them v_mad_u64_u32)",
                "hbm": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                        "algorithmic_bytes_per_launch": alg_bytes, "note": "128 B per (point, scalar) pair / the kernel's HIP-event time (SURVEY.md 8d)"},
            },
        }

    emit_lock, emitted = threading.Lock(), [False]

    def emit():
        with emit_lock:
            if rank == 0 and not emitted[0]:
                emitted[0] = True
                print(json.dumps(out), flush=True)

    def on_deadline():
        if rank == 0:
            out["extras_incomplete"] = "deadline reached: the legs after the headline did not finish"
        emit()
        os._exit(0)

    watchdog = threading.Timer(float(os.environ.get("ZK_BENCH_DEADLINE_S", "900" if world == 1 else "420")), on_deadline)
    watchdog.daemon = True
    if rank == 0 or isinstance(grp, ProcGroup):  # (party threads share one process: rank 0's timer speaks for all)
        watchdog.start()

    extra = {}
    # ---- the north-star size: collaborative HyperPlonk l = 1, n = 24 (BASELINE configs[4]: one party's full work on one GPU) ----
    # from the compiled host in its own process, self-checked by the host's own anchored verifier.  It runs BEFORE the other legs:
    # the n = 24 parameter set with its window tables and pass arenas wants most of the device, and this process holds only the
    # headline's 2^20-point level at this point.  Skipped -- and said so -- when the free HBM is below the footprint.
    if world == 1 and extra_legs and not args.no_e2e and not args.no_e2e_n24:
        try:
            ctx.trim()
            free_b, total_b = ctx.mem_info()
            need_b = 200 << 30
            if free_b < need_b:
                extra["e2e_n24"] = {"skipped": f"{free_b >> 30} GiB of HBM free, the n = 24 parameter set with its window tables and pass arenas wants ~{need_b >> 30} GiB"}
            else:
                plan24 = os.path.join(ROOT, "gpurun_out", ".arena_plan_n24.bin")
                os.makedirs(os.path.dirname(plan24), exist_ok=True)
                if os.path.exists(plan24):
                    os.remove(plan24)
                r24 = cpp_host_e2e(24, reps=2, check=True, serial_rep=True, timeout=1500, arena_plan=plan24)
                # a second process of the same prover with the arena plan the first one left (zk_arena_plan_import right after the setup):
                # its FIRST proof allocates nothing -- what a deployment that keeps the plan beside its proving key sees
                if "error" not in r24 and os.path.exists(plan24):
                    again = cpp_host_e2e(24, reps=2, timeout=900, arena_plan=plan24)
                    t_first, t_best = again.get("first_proof_s"), (again.get("timers_s") or {}).get("Distributed HyperPlonk")
                    r24["second_process_with_arena_plan"] = {"first_proof_s": t_first, "steady_proof_s": t_best, "first_over_steady": (t_first / t_best) if t_first and t_best else None,
                                                             "arena_plan": again.get("arena_plan"), "error": again.get("error")}
                # the driver returns the child's ~200 GiB of HBM asynchronously after its exit: wait until this process sees them again
                # (an allocation of the next leg right behind the child's exit was refused once the tables grew to 128-B records)
                t_w = time.perf_counter()
                while time.perf_counter() - t_w < 60.0:
                    if ctx.mem_info()[0] >= free_b - (8 << 30):
                        break
                    time.sleep(0.25)
                r24["hbm_back_after_s"] = time.perf_counter() - t_w
                ref24 = 398458791  # SURVEY.md 8(d), derived from dhyperplonk.rs:198-553
                comp24 = ref24 - (1 << 25)  # the two opens of V share their first quotient's commitment (computed once)
                t24 = (r24.get("timers_s") or {}).get("Distributed HyperPlonk")
                r24.update({"n": 24, "l": 1, "parties": 8, "mode": "leader (party 0's full work, no-comm echo net), compiled C++ host, own process",
                            "parameter_set": "SplitMix64 tables (seed 100), challenges 4242", "hbm_free_before_GiB": free_b >> 30,
                            "scalar_muls_per_proof_reference_count": ref24, "scalar_muls_computed": comp24,
                            "scalar_muls_computed_per_s": (comp24 / t24) if t24 else None})
                extra["e2e_n24"] = r24
        except Exception as ex:
            extra["e2e_n24"] = {"error": repr(ex)}

    if extra_legs:
        try:
            # ---- strong scaling of ONE primitive over the ranks (total work fixed) ----
            strong = {}
            big = args.big
            for lg in (args.log2n, big):
                per = (1 << lg) // world
                s_srs = ctx.srs_generate(0xABCDE, 0x13579, 1 << lg) if world == 1 else ctx.srs_generate(0xABCDE + per * rank * 0x13579, 0x13579, per)
                if not args.no_precompute:
                    s_srs.precompute(0, record_bytes=args.table_rec)  # (setup, like the headline's)
                s_sc = device_table(ctx, max(lg - (world.bit_length() - 1), 0), 77 + rank)
                fn = (lambda: ctx.msm_g1(s_srs, s_sc, per)) if world == 1 else (lambda: sh.sharded_msm(ctx, s_srs, s_sc, per, net))
                for _ in range(3 if lg <= 20 else 1):  # (like the headline's warm-up: the first calls on a new level also size the arenas)
                    fn()
                tt = timed(fn, 10 if lg <= 20 else 2, barrier)
                strong[f"msm_2p{lg}"] = {"ms": tt * 1e3, "scalar_muls_per_s": (1 << lg) / tt, "points_per_rank": per, "srs_window_table_bits": s_srs.table_window}
                if lg == big and lg != args.log2n and rank == 0:
                    # roofline of the dominant kernel at the north-star size (2^24 points; this rank's chunk at N > 1), same model as the headline's
                    k_ms = float(ctx.msm_last_timing()[1])
                    tcb = s_srs.table_window
                    cb = tcb or ctx.lib.zk_msm_window(per)
                    wins, ents = ((256 + cb - 1) // cb, per) if tcb else ((129 + cb - 1) // cb, 2 * per)
                    md = float(wins) * ents
                    tr24, src24 = pmc_traffic("k_accum_tiles", "largest_grid") if (world == 1 and lg == 24 and not args.no_precompute) else (None, None)
                    extra[f"roofline_msm_2p{lg}"] = {
                        "kernel": "zk::k_accum_tiles (bucket accumulation)", "points": per, "bound": "int_alu", "kernel_ms": k_ms, "pippenger_window_bits": cb, "windows": wins,
                        "achieved": md * MADS_PER_MADD / (k_ms * 1e-3) / 1e12 if k_ms > 0 else 0.0, "peak": MAD_PEAK / 1e12, "unit": "T v_mad_u64_u32/s",
                        "frac": md * MADS_PER_MADD / (k_ms * 1e-3) / MAD_PEAK if k_ms > 0 else 0.0,
                        "frac_of_architectural": md * MADS_PER_MADD / (k_ms * 1e-3) / MAD_PEAK_ARCH if k_ms > 0 else 0.0,
                        "traffic": tr24, "traffic_source": src24,
                        "hbm": {"bound": "hbm", "achieved": 128.0 * per / (k_ms * 1e-3) / 1e9 if k_ms > 0 else 0.0, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                "frac": 128.0 * per / (k_ms * 1e-3) / 1e9 / HBM_PEAK_GBS if k_ms > 0 else 0.0, "algorithmic_bytes_per_launch": 128.0 * per}}
                    if tcb:
                        # the HBM-bound phase of the MSM: signed digits + the two-level counting sort (round 6: k_tab_hist, k_tab_scatter, k_l2_*).
                        # Algorithmic bytes: 32 B per scalar in, 4 B per sorted entry out; live time = HIP events around the phase
                        # (zk_msm_last_timing[0]); traffic = FETCH_SIZE x 2 + WRITE_SIZE of the phase's kernels from the committed PMC passes
                        s_ms = float(ctx.msm_last_timing()[0])
                        alg = 32.0 * per + 4.0 * md
                        tr_s, src_s = sort_phase_traffic() if (world == 1 and lg == 24) else (None, None)
                        extra[f"roofline_msm_2p{lg}"]["sort_phase"] = {
                            "kernels": "k_tab_hist, k_part_scan, k_part_bases, k_tab_scatter, k_l2_tiles, k_l2_hist, k_l2_scan, k_l2_scatter", "bound": "hbm", "phase_ms": s_ms,
                            "algorithmic_bytes": alg, "achieved": alg / (s_ms * 1e-3) / 1e9 if s_ms > 0 else 0.0, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                            "frac": alg / (s_ms * 1e-3) / 1e9 / HBM_PEAK_GBS if s_ms > 0 else 0.0, "traffic": tr_s, "traffic_source": src_s,
                            "traffic_GBps": (tr_s / (s_ms * 1e-3) / 1e9) if (tr_s and s_ms > 0) else None,
                            "note": "every kernel of the phase moves its own algorithmic bytes (profiles/r06z_sort_phase_pmc.csv); the phase as a whole moves ~4x the compulsory "
                                    "bytes because the scalars are read twice and the 6-byte level-1 entries make one round trip (DESIGN.md section 4)"}
                s_srs.free()
                del s_sc
            per = (1 << big) // world
            sf, sg = device_table(ctx, big - (world.bit_length() - 1), 5 + rank), device_table(ctx, big - (world.bit_length() - 1), 105 + rank)
            fn = (lambda: ctx.sumcheck_product(sf, sg, per, chal)) if world == 1 else (lambda: sh.sharded_sumcheck_product(ctx, sf, sg, per, chal[:big], net))
            fn()
            tt = timed(fn, 5, barrier)
            strong[f"sumcheck_product_2p{big}"] = {"ms": tt * 1e3, "fr_field_ops_per_s": 18.0 * (1 << big) / tt, "hbm_algorithmic_GBps": 64.0 * (1 << big) / tt / 1e9,
                                                  "elements_per_rank": per, "layout": "cyclic (index i on rank i mod N)"}
            extra["strong"] = dict(strong, note="total size fixed, split over the ranks; N = 1 is the monolithic call")
            r24 = extra.get("e2e_n24") or {}
            single = (strong.get("msm_2p24") or {}).get("scalar_muls_per_s")  # one blocking 2^24-point MSM of this run
            if r24.get("scalar_muls_computed_per_s") and single:
                r24["fraction_of_single_2p24_msm_rate"] = r24["scalar_muls_computed_per_s"] / single

            # ---- the sumcheck family against the HBM roofline (rank-local; reported at N = 1) ----
            if world == 1:
                sc = {}
                for lg in (args.log2n, big, big + 2):
                    m = 1 << lg
                    f_t = sf if lg == big else device_table(ctx, lg, 11)
                    g_t = sg if lg == big else device_table(ctx, lg, 12)
                    q_t, o_t = ctx.alloc(32 * m), ctx.alloc(32)
                    row = {}
                    for name, fn, byt, ops in (("product", lambda: ctx.sumcheck_product(f_t, g_t, m, chal), 64, 18.0), ("plain", lambda: ctx.sumcheck(f_t, m, chal), 32, 5.0),
                                               ("fold", lambda: (ctx.fold(f_t, m, chal[:lg], out=o_t), ctx.sync()), 32, 3.0), ("open", lambda: ctx.open_rounds(f_t, m, chal, q_out=q_t), 64, 4.0)):
                        fn()
                        tt = timed(fn, 10 if lg <= 22 else 3, barrier)
                        row[name] = {"ms": tt * 1e3, "hbm_algorithmic_GBps": byt * m / tt / 1e9, "hbm_frac": byt * m / tt / 1e9 / HBM_PEAK_GBS, "fr_field_ops_per_s": ops * m / tt}
                    sc[f"2p{lg}"] = row
                    del q_t
                    if lg != big:
                        del f_t, g_t
                sc["note"] = ("algorithmic bytes: product 64 N, plain 32 N, fold 32 N, open 64 N (SURVEY.md 8d model A); field-op counts as the reference writes them "
                              "(product 9N mul + 9N add; plain 2N + 3N).  fold and plain run as flat linear passes (one wide multiply-accumulate per element): HBM-bound; "
                              "the product sumcheck (2 wide accumulations + 2 multiplications per pair) is bound by the integer multiplier's issue rate")
                # roofline of the product sumcheck's dominant kernel, k_pass<2,1> (first HBM pass of the call: two rounds fused in
                # registers), HIP events on the ctx stream (zk_sumcheck_last_timing).  Per lane iteration (4 + 4 elements in, one
                # pair out): three pair-rounds of 2 wide accumulations (64 mad) + 2 multiplications (128 mad), + 2 wide accumulations
                # for the t1 of the call's first round.
                try:
                    ctx.dbg_tune("sc_ts", 3)
                    kp = {}
                    for lg in (args.log2n, big, big + 2):
                        m = 1 << lg
                        f_t, g_t = device_table(ctx, lg, 11), device_table(ctx, lg, 12)
                        ts = []
                        for _ in range(6):
                            ctx.sumcheck_product(f_t, g_t, m, chal)
                            ts.append(ctx.sumcheck_last_timing().copy())
                        first_ms, all_ms = [float(x) for x in np.median(np.array(ts[1:]), axis=0)]
                        mads = (m / 4) * (3 * (2 * 64 + 2 * 128) + 2 * 64)
                        kp[f"2p{lg}"] = {"kernel": "zk::k_pass<2, 1> (first pass)", "kernel_ms": first_ms, "all_launches_ms": all_ms,
                                         "bound": "int_alu", "achieved": mads / (first_ms * 1e-3) / 1e12, "peak": MAD_PEAK / 1e12, "unit": "T v_mad_u64_u32/s",
                                         "frac": mads / (first_ms * 1e-3) / MAD_PEAK,
                                         "hbm": {"achieved": 64.0 * m / (first_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": 64.0 * m / (first_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                                 "note": "the pass reads both tables once (64 B per index pair of the call's algorithmic bytes)"}}
                        del f_t, g_t
                    sc["roofline_k_pass"] = kp
                finally:
                    ctx.dbg_tune("sc_ts", 0)
                # the same calls timed FROM C (tests/native/sc_latency.c, plain C over include/zkhip.h): the figures above go through
                # the Python wrapper, which allocates four numpy arrays and converts eight ctypes arguments per call (7 us at 2^20)
                try:
                    import subprocess

                    exe = os.path.join(ROOT, "tests", "native", "sc_latency")
                    if os.path.exists(exe):
                        ctx.sync()
                        txt = subprocess.run([exe, str(args.log2n)], capture_output=True, text=True, timeout=120).stdout
                        cabi = {}
                        for line in txt.splitlines():
                            w = line.split()
                            if len(w) > 6 and w[2] == "mean":
                                cabi[w[0]] = {"mean_us": float(w[3]), "min_us": float(w[6])}
                        sc["c_abi_2p%d" % args.log2n] = dict(cabi, note="wall time per call measured from a plain-C caller of the C ABI (200 calls after 5 warm-up calls), own process and ctx")
                except Exception as ex:
                    sc["c_abi_error"] = repr(ex)
                extra["sumcheck"] = sc
                # the sumcheck half of the metric as a named top-level field (BASELINE configs[2]: 20-variate over 2^20 Fr shares)
                r20 = sc.get(f"2p{args.log2n}", {})
                if r20:
                    m20 = float(1 << args.log2n)
                    cab = sc.get("c_abi_2p%d" % args.log2n, {})
                    call_s = {k: (cab[k]["mean_us"] * 1e-6 if k in cab else r20[k]["ms"] * 1e-3) for k in ("product", "plain") if k in r20}
                    # arithmetic the library really performs per call: product = per pair and round 2 wide accumulations (64 mad each) + 2 Montgomery
                    # multiplications (128 mad each), pairs over all rounds = m - 1, + the first round's t1 (64 mad per pair of m / 2); plain (flat
                    # passes) = one wide multiply-accumulate (64 mad) per element
                    mads = {"product": (m20 - 1) * (2 * 64 + 2 * 128) + 64 * m20 / 2, "plain": 64 * m20}
                    extra["d_sumcheck"] = {
                        "metric": f"Fr field-ops/s (d_sumcheck), 2^{args.log2n} Fr shares, {args.log2n}-variate (BASELINE configs[2])",
                        "value": 18.0 * m20 / call_s["product"], "unit": "Fr field-ops/s",
                        "count": "as the reference writes the loops: sumcheck_product 9N mul + 9N add per call (dsumcheck.rs:37-85); plain sumcheck 2N mul + 3N add (dsumcheck.rs:10-21)",
                        "sumcheck_product": {"us_per_call": call_s["product"] * 1e6, "fr_field_ops_per_s": 18.0 * m20 / call_s["product"]},
                        "sumcheck": {"us_per_call": call_s["plain"] * 1e6, "fr_field_ops_per_s": 5.0 * m20 / call_s["plain"]},
                        "timed_at": "the C ABI from a plain-C caller (tests/native/sc_latency.c)" if cab else "the Python wrapper",
                        "roofline": {name: {"bound": "latency chain (one Fr multiplication per round) below int_alu / hbm at this size", "call_us": call_s[name] * 1e6,
                                            "hbm": {"achieved": byt * m20 / call_s[name] / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": byt * m20 / call_s[name] / 1e9 / HBM_PEAK_GBS,
                                                    "algorithmic_bytes_per_call": byt * m20},
                                            "int_alu": {"achieved": mads[name] / call_s[name] / 1e12, "peak": MAD_PEAK / 1e12, "unit": "T v_mad_u64_u32/s", "frac": mads[name] / call_s[name] / MAD_PEAK,
                                                        "frac_of_architectural": mads[name] / call_s[name] / MAD_PEAK_ARCH}}
                                     for name, byt in (("product", 64.0), ("plain", 32.0)) if name in call_s}}
            del sf, sg
            ctx.trim()

        except Exception as ex:  # the contract line must survive a failure of these legs
            extra["legs_error"] = repr(ex)

        # ---- end to end: collaborative HyperPlonk l = 1, n = 20 (BASELINE configs[3]) ----
        if world in (1, 8) and not args.no_e2e:
            try:
                import zkhip.dist_primitive as _dp
                from zkhip.hyperplonk import PackedProvingParameters, dhyperplonk
                from zkhip.net import LeaderEchoNet
                from zkhip.pss import PackedSharingParams
                from zkhip.verify import check_closing_rows, check_dhyperplonk_transcripts, dhyperplonk_anchors, trace_anchor_values

                e_n = args.e2e_n
                e_pp = PackedSharingParams(1)
                e_net = net if world == 8 else LeaderEchoNet(8)
                t0 = time.perf_counter()
                # the SplitMix64 parameter set (SURVEY.md 8(d) "Synthetic inputs") that the C++ host builds as well: per-party tables
                # (seed 100 + party), shared public challenges
                pk = PackedProvingParameters.new_splitmix(e_n, e_pp, ctx, seed=100 + rank, chal_seed=4242)
                setup_s = time.perf_counter() - t0
                TOT = "Distributed HyperPlonk"

                def best_of(reps):
                    best = None
                    for _ in range(reps):
                        _, tm = dhyperplonk(e_n, pk, e_pp, ctx, e_net, seed=7 + rank)
                        if best is None or tm.get(TOT, 1e9) < best.get(TOT, 1e9):
                            best = tm
                    return best

                best = best_of(4)
                # the driver computes identical MSM items of a step once (the two c_opens of V, dhyperplonk.rs:307-320, commit the
                # same first quotient: 2^(n+1) of the proof's scalar-muls); the figure without that sharing is reported beside it
                _dp.DEDUP_MSM = False
                try:
                    plain = best_of(2)
                finally:
                    _dp.DEDUP_MSM = True
                # ... and with the MSM pass of every step run to completion inside its own step (no start / finish overlap): only
                # in this form do the per-step timers cover what the reference's log labels cover
                _dp.PIPELINE_MSM = False
                try:
                    serial = best_of(2)
                finally:
                    _dp.PIPELINE_MSM = True
                # self-check of the reported run AT EVERY N: every transcript's verifier chain with both ends pinned by values
                # computed through other kernels (claim sum f g: zk_fr_mul + the plain sumcheck's first round; final evaluation:
                # two zk_fold) -- zkhip.verify.  The leader's d_sumcheck_product chains need every party's values (sums of the
                # claims, the fold of the parties' last values, dsumcheck.rs:440-507): one all-gather of a few Fr per transcript,
                # outside the timed region.  The closing row of every c_sumcheck_product is compared with pss2ss of the
                # independently folded last values (dsumcheck.rs:224-225,282).
                ctx.sc_trace = []
                res, _ = dhyperplonk(e_n, pk, e_pp, ctx, e_net, seed=7 + rank)
                trace, ctx.sc_trace = ctx.sc_trace, None
                mine = trace_anchor_values(ctx, trace)
                del trace
                values = grp.all_gather_obj(mine) if world == 8 else [mine]
                anchors = dhyperplonk_anchors(values, rank if world == 8 else 0, 8)
                bad = list(check_dhyperplonk_transcripts(e_n, res, pk, 8, e_net.is_leader, world == 1, anchors=anchors))
                want = len(mine) if e_net.is_leader else 7
                if len(anchors) != want:
                    bad.append(f"{len(anchors)} anchors instead of {want}")
                if not check_closing_rows(mine[:7], list(res[0][0]) + [res[1][0][0]], e_pp, e_net):
                    bad.append("closing row of a c_sumcheck_product differs from pss2ss of the folded last values")
                bad_all = [f"party {p}: {b}" for p, bs in enumerate(grp.all_gather_obj(bad)) for b in bs] if world == 8 else bad
                ref_count = {12: 97227, 20: 24903603, 24: 398458791}.get(e_n)  # SURVEY.md 8(d), derived from dhyperplonk.rs:198-553
                computed = (ref_count - (1 << (e_n + 1))) if ref_count else None
                e_digest = transcript_sha256(res) if rank == 0 else None  # (world 8: the leader's transcript)
                extra["e2e"] = {"n": e_n, "l": 1, "parties": 8, "parameter_set": "SplitMix64 tables (seed 100 + party), challenges 4242", "transcript_sha256": e_digest, "mode": "leader (party 0's full work, no-comm echo net)" if world == 1 else f"8 parties = 8 ranks, exchanges: {type(e_net).__name__} ({backend})",
                                "setup_s": setup_s, "timers_s": best,
                                "timers_note": "the MSM pass of a step is started asynchronously and collected later (MsmQueue.start / finish); the kernel phase of the Open step runs before the wiring "
                                               "pass is started so that both passes are in flight back to back: 'Commit' / 'Wire identity' / 'Open' are OVERLAPPED sections that no longer cover the "
                                               "reference's steps, only the total is comparable with the reference's log; timers_s_serial_steps runs every pass to completion where it is started",
                                "timers_s_serial_steps": serial,
                                "scalar_muls_per_proof_reference_count": ref_count,
                                "scalar_muls_computed": computed,
                                "scalar_muls_computed_per_s": (computed / best[TOT]) if (computed and best and best.get(TOT)) else None,
                                "scalar_muls_note": "the two opens of V commit the same first quotient (2^(n+1) scalar-muls): computed once here, twice in the reference; rates use the COMPUTED count",
                                "timers_s_every_msm_separately": plain, "transcript_checks": "ok" if not bad_all else bad_all,
                                "transcript_check_kind": "anchored: both ends of every chain pinned by independent kernels (claim + final evaluation), closing rows against pss2ss of independent folds"
                                                         + ("; the leader's d_ chains by all 8 parties' gathered values" if world == 8 else "")}
                if bad_all:
                    extra["e2e"]["timers_s"] = None  # an unverified figure is not a figure
                del pk
                ctx.trim()
            except Exception as ex:  # the headline must survive a failure of this leg
                extra["e2e"] = {"error": repr(ex)}
            if world == 1 and isinstance(extra.get("e2e"), dict) and "error" not in extra["e2e"]:
                extra["e2e"]["cpp_host"] = cpp_host_e2e(args.e2e_n, want_digest=extra["e2e"].get("transcript_sha256") if extra["e2e"].get("transcript_checks") == "ok" else None, check=True,
                                                        serial_rep=True)
                # one figure per proof: the faster of the two verified hosts (same inputs, same transcript)
                cand = {"python": (extra["e2e"].get("timers_s") or {}).get("Distributed HyperPlonk"),
                        "cpp": (extra["e2e"]["cpp_host"].get("timers_s") or {}).get("Distributed HyperPlonk") if extra["e2e"]["cpp_host"].get("transcript_equals_python_host") else None}
                cand = {k: v for k, v in cand.items() if v}
                if cand:
                    best_host = min(cand, key=cand.get)
                    extra["e2e"]["proof_s"] = {"host": best_host, "seconds": cand[best_host], "all": cand}
                    comp = extra["e2e"].get("scalar_muls_computed")
                    if comp and out.get("value"):
                        # how close the proof's mix of 794 MSMs (2^10 .. 2^22 points) runs to the rate of ONE 2^20-point MSM (`value`)
                        extra["e2e"]["msm_mix_efficiency"] = {"proof_scalar_muls_per_s": comp / cand[best_host], "single_2p20_msm_scalar_muls_per_s": out["value"],
                                                              "ratio": comp / cand[best_host] / out["value"],
                                                              "note": "scalar-muls the proof computes / its wall time (sumchecks, exchanges and host arithmetic included), over the headline rate"}

        # ---- the collaborative permutation check alone (dhyperplonk.rs:1249-1385; north_star "dperm/cperm"), n = e2e_n, l = 1, compiled host ----
        if world == 1 and not args.no_e2e and not args.no_extra:
            try:
                ctx.trim()
                cp = cpp_host_e2e(args.e2e_n, reps=3, check=True, which="cpermcheck", timeout=600)
                if "error" not in cp and cp.get("timers_s"):
                    g4 = 4 << args.e2e_n
                    cp["scalar_muls_reference_count"] = 22 * g4 - 12  # 10 c_commit of 4 * 2^n scalars + 12 c_open of 4 * 2^n - 1 quotient scalars
                    cp["scalar_muls_computed"] = 20 * g4 - 10           # the repeated opens of num / den (:1324, :1371: same table, same point) are computed once
                    cp["scalar_muls_computed_per_s"] = cp["scalar_muls_computed"] / cp["timers_s"]["Collaborative Permcheck"]
                    cp["schedule"] = "the two masked product trees, then ONE MSM pass over all commitments / quotient commitments and one batch of the opens' fold rounds + the six product sumchecks"
                extra["cpermcheck"] = cp
            except Exception as ex:
                extra["cpermcheck"] = {"error": repr(ex)}

        # ---- N = 8: the same proofs from the COMPILED host over RCCL (BASELINE configs[3] and configs[4]) ----
        # hyperplonk --mode rccl is ONE process that drives all 8 GPUs (zk_comm_init_all, a host thread per party): rank 0 starts it
        # while the ranks of this bench wait at a barrier with their arenas trimmed.  Every party checks its own transcripts
        # (zkhost/verify.hpp) and the digest must equal the Python host's over the same nets.  ZK_BENCH_CPP_RCCL=share runs the
        # leg with --share-gpus on a box with fewer GPUs (functional: only the test double of librccl accepts that).
        cpp_rccl = os.environ.get("ZK_BENCH_CPP_RCCL", "auto")
        if world == 8 and not args.no_e2e and cpp_rccl != "0" and (backend in ("nccl", "rccl") or cpp_rccl == "share"):
            try:
                barrier()
                if rank == 0:
                    leg = {}
                    for e_n in ((args.e2e_n,) if (args.no_e2e_n24 or cpp_rccl == "share") else (args.e2e_n, 24)):
                        py = extra.get("e2e") or {}
                        leg[f"n{e_n}"] = cpp_host_e2e(e_n, reps=3 if e_n <= 20 else 2, check=True, mode="rccl", share_gpus=cpp_rccl == "share", timeout=900,
                                                      want_digest=py.get("transcript_sha256") if (e_n == py.get("n") and py.get("transcript_checks") == "ok") else None)
                    leg["note"] = ("'Distributed HyperPlonk' of timers_s is the leader's wall time of one proof with all 8 parties running; "
                                   "self_check lists every party's verdict; a run whose check fails has timers_s = null")
                    extra["e2e_cpp_rccl"] = leg
                barrier()
            except Exception as ex:
                extra["e2e_cpp_rccl"] = {"error": repr(ex)}

        # ---- G2: `d_msm` is generic over CurveGroup (dmsm.rs:9), powers_of_g2 are G2 points (dpoly_comm.rs:27,59-62) ----
        if world == 1:
            try:
                from zkhip import pairing as pr
                from zkhip.field import fq_mont

                g_lg = 17
                g_n = 1 << g_lg
                stp, cur, rows = pr.g2_mul(pr.G2_GEN, 991), pr.g2_mul(pr.G2_GEN, 77), []
                for _ in range(g_n):  # an arithmetic sequence of G2 points (host big-int arithmetic, setup only)
                    rows.append(np.concatenate([fq_mont(cur[0][0]), fq_mont(cur[0][1]), fq_mont(cur[1][0]), fq_mont(cur[1][1])]))
                    cur = pr.g2_add(cur, stp)
                g_srs = ctx.srs_register_g2(np.array(rows, dtype=np.uint64))
                g_sc = ctx.to_device(random_fr(g_n, seed + 9))
                ref = ctx.msm_g2(g_srs, g_sc, g_n)
                t_plain = timed(lambda: ctx.msm_g2(g_srs, g_sc, g_n), 5, barrier)
                g_srs.precompute(0)
                same = bool((ctx.msm_g2(g_srs, g_sc, g_n) == ref).all())
                t_tab = timed(lambda: ctx.msm_g2(g_srs, g_sc, g_n), 10, barrier)
                ph = ctx.msm_last_timing()
                extra["g2"] = {"points": g_n, "scalar_muls_per_s": g_n / t_tab, "ms": t_tab * 1e3, "srs_window_table_bits": g_srs.table_window,
                               "without_window_table": {"scalar_muls_per_s": g_n / t_plain, "ms": t_plain * 1e3},
                               "same_result_with_and_without_table": same,
                               "phase_ms": {"digits_sort": float(ph[0]), "k_accum_tiles": float(ph[1]), "fixup": float(ph[2]), "bucket_reduce": float(ph[3]), "host_combine": float(ph[4])},
                               "note": "coordinates in Fq2: one multiplication = two fused two-product Montgomery multiplications (1014 mad vs 338 in G1), 256-bit scalars (no endomorphism split)"}
                g_srs.free()
            except Exception as ex:
                extra["g2"] = {"error": repr(ex)}

        # second figure: the same step with the scalars coming from host memory (PCIe-inclusive); never `value`
        if world == 1:
            tmp = ctx.alloc(32 * n)

            def h2d_step():
                tmp.upload(scal_np)
                ctx.msm_g1(srs, tmp, n)

            h2d_step()
            extra["ms_per_step_scalars_from_host"] = timed(h2d_step, 3, barrier) * 1e3

    if rank != 0:
        watchdog.cancel()
        grp.finish()
        return

    out.update(extra)

    if args.full and not args.no_cpu and world == 1:  # the CPU leg runs at N = 1 only (rank 0)
        # CPU baseline leg: the oracle (C port of the reference's single-threaded path) on this
        # box's host cores.  Checker/baseline only -- never part of the measured GPU path.
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import coracle as co

        m = 1 << args.cpu_log2n
        bases_h = srs.download()[:m].copy()
        sc_h = scal_np[:m].copy()
        t = time.perf_counter()
        ref = co.msm_g1(bases_h, sc_h)
        cpu_dt = time.perf_counter() - t
        got = ctx.msm_g1(srs, ctx.to_device(sc_h), m)
        assert (got[:12] == ref).all(), "GPU MSM differs from the CPU oracle on the baseline sample"
        # BASELINE configs[2] on its own size: the 20-variate product sumcheck (two tables of 2^20 Fr), checked against the GPU transcript
        f_h, g_h = random_fr(1 << 20, 1), random_fr(1 << 20, 2)
        t = time.perf_counter()
        sc_ref = co.sumcheck_product(f_h, g_h, chal[:20])
        cpu_sc = time.perf_counter() - t
        sc_got = ctx.sumcheck_product(ctx.to_device(f_h), ctx.to_device(g_h), 1 << 20, chal[:20])[0]
        assert (np.asarray(sc_got) == sc_ref[:20]).all(), "GPU product sumcheck differs from the CPU oracle on the baseline sample"
        # generous baseline: the same port on many host cores (the reference itself is single-threaded per
        # party: no `parallel` feature, Cargo.lock:120-134) -- contiguous chunks of the MSM on a thread
        # pool (ctypes releases the GIL), partial results added with the oracle's group law
        from concurrent.futures import ThreadPoolExecutor

        cores = max(1, min(64, (os.cpu_count() or 1) // 2))
        bounds = [m * i // cores for i in range(cores + 1)]
        t = time.perf_counter()
        with ThreadPoolExecutor(cores) as ex:
            parts = list(ex.map(lambda i: co.msm_g1(bases_h[bounds[i] : bounds[i + 1]], sc_h[bounds[i] : bounds[i + 1]]), range(cores)))
        import pyoracle as po
        from zkhip.field import affine_mont_to_ints

        acc = None
        for pt in parts:
            acc = po.g1_add(acc, affine_mont_to_ints(pt))
        cpu_mt = time.perf_counter() - t
        assert acc == affine_mont_to_ints(ref), "chunked CPU MSM differs from the single-thread result"
        # anchor to the reference's own numbers: its sample log times party 0's local MSM inside c_commit -- 1 024 points, single
        # thread, ark-ec on an unnamed host -- at 18.5-19.5 ms (hack/run-hyperplonk/output.txt:22-23,34-35).  The same size through the port:
        t = time.perf_counter()
        for _ in range(20):
            co.msm_g1(bases_h[:1024], sc_h[:1024])
        cpu_1k = (time.perf_counter() - t) / 20
        out["cpu_baseline"] = {
            "reference_log_anchor": {"points": 1024, "port_ms": cpu_1k * 1e3, "reference_ms": [18.5, 19.5], "port_over_reference": cpu_1k * 1e3 / 19.0,
                                     "note": "the reference's leader log (hack/run-hyperplonk/output.txt:22-23,34-35: 'Local: MSM' of c_commit, one thread, host not named; 2^10 points -- the "
                                             "log's c_open batches ten commitments, :565, i.e. 2^10-element share tables) beside the C port on this box at the same size: where the ratio is "
                                             "above 1 the real ark-ec path is that much faster per core than the port, and the CPU baseline figures should be read with that factor"},
            "value": m / cpu_dt,
            "unit": "G1 scalar-muls/s",
            "cores": 1,
            "kind": "port",
            "sample": f"one MSM of 2^{args.cpu_log2n} of the same bases/scalars (ark-ec window rule c={co.msm_window(m)}), {cpu_dt:.1f} s; result bit-identical to the GPU",
            "sumcheck_fr_field_ops_per_s": 18.0 * (1 << 20) / cpu_sc,
            "sumcheck_sample": f"sumcheck_product on 2^20 random Fr (the size of BASELINE configs[2]), {cpu_sc:.2f} s; transcript bit-identical to the GPU's",
            "all_cores": {"value": m / cpu_mt, "unit": "G1 scalar-muls/s", "cores": cores, "sample": f"same MSM in {cores} chunks on {cores} threads, {cpu_mt:.2f} s"},
            "host": os.uname().nodename,
            "cpu_model": next((ln.split(":", 1)[1].strip() for ln in open("/proc/cpuinfo") if ln.startswith("model name")), "unknown") if os.path.exists("/proc/cpuinfo") else "unknown",
            "nproc": os.cpu_count(),
        }
        # end-to-end denominator: the SAME dhyperplonk call sequence through the C port (one thread, one party's
        # work, leader mode) at a size the time box allows; larger sizes are extrapolated by scalar-mul count at
        # the measured single-thread 2^20 MSM rate, which FLATTERS the CPU (most MSMs of the sequence are smaller
        # and run at a lower rate per point) -- the stated speed-ups are therefore lower bounds
        try:
            from oracle_backend import OracleBackend
            from zkhip.hyperplonk import PackedProvingParameters, dhyperplonk
            from zkhip.net import LeaderEchoNet
            from zkhip.pss import PackedSharingParams

            cn = args.cpu_e2e_n
            obe, opp = OracleBackend(), PackedSharingParams(1)
            opk = PackedProvingParameters.new(cn, opp, obe, seed=1)
            t = time.perf_counter()
            dhyperplonk(cn, opk, opp, obe, LeaderEchoNet(8), seed=2)
            cpu_e2e = time.perf_counter() - t
            rate = m / cpu_dt
            muls = lambda k: 23.75 * (1 << k)  # scalar-muls per proof: 97 227 / 24 903 603 / 398 458 791 at n = 12 / 20 / 24
            e = {"n": cn, "seconds": cpu_e2e, "cores": 1, "kind": "port", "sample": f"dhyperplonk leader mode, n = {cn}, C port behind the same host driver",
                 "extrapolated_s_lower_bound": {"n20": muls(20) / rate, "n24": muls(24) / rate},
                 "extrapolated_s_scaled_sample": {"n20": cpu_e2e * muls(20) / muls(cn), "n24": cpu_e2e * muls(24) / muls(cn)},
                 "extrapolation": "lower bound = scalar-mul count of the proof / the single-thread 2^20 MSM rate above (MSM only, at the best per-point rate); "
                                  "scaled sample = the measured run x the ratio of scalar-mul counts (keeps the small-MSM inefficiency of the sample: an upper estimate)"}
            if "e2e" in out and out["e2e"].get("timers_s"):
                e["gpu_n20_speedup_lower_bound"] = e["extrapolated_s_lower_bound"]["n20"] / out["e2e"]["timers_s"]["Distributed HyperPlonk"]
            out["cpu_baseline"]["e2e"] = e
        except Exception as ex:
            out["cpu_baseline"]["e2e"] = {"error": repr(ex)}
    watchdog.cancel()
    emit()
    grp.finish()


if __name__ == "__main__":
    main()
