#!/usr/bin/env python3
"""End-to-end rate of PTABlockGibbs.sample() on the 45-pulsar array: sweeps, recording and files.

    python tools/sample_rate.py --kind curn_red --nchains 2048 --niter 501 \\
        --runs bare,memory,disk8,disk8-device,diskall,diskall-device --out profiles/sample_stream/curn_red.json

Runs (each a fresh PTABlockGibbs on one synthetic.array_pta(kind, n_psr) model):
  bare            eng.sweep() in a loop, nothing recorded, one synchronise per save_every sweeps
  memory          sample(history="memory"): the default mode (eager sweeps, host history, files
                  rewritten at every save point)
  diskK[-device]  sample(history="disk", record_chains=K or all): graph replays, block record
                  into pinned host slots (or HBM slots copied by a side stream: -device)
  summaryK        sample(history="summary", record_chains=K): the disk path keeping K chains, plus
                  every chain's posterior summary accumulated on the device (summary.npz)

Timing: wall clock between the save points sample() reports ("Finished ... percent"), i.e. whole
blocks of save_every sweeps with their recording and file work.  The first block (sweep 0, graph
capture, code loading) is the warm block and is excluded; the median and the spread of the rest
are reported, next to the wall time of the whole call.  The disk mode reports a block when it is
fetched, one block behind its launch: the intervals still are one block each.
Needs a GPU; there is no CPU fallback.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class SavePointClock:
    """stdout stand-in that notes the time of every progress report of sample()."""

    def __init__(self, out):
        self.out, self.t = out, []

    def write(self, s):
        if s.startswith("Finished "):
            self.t.append(time.perf_counter())
        return len(s)

    def flush(self):
        pass


def block_stats(t, save_every, nchains):
    d = np.diff(np.asarray(t))         # t[0] ends the warm block: no interval contains it
    if d.size == 0:
        return {"blocks": 0}
    med = float(np.median(d))
    return {"blocks": int(d.size), "block_s_median": med, "block_s_min": float(d.min()),
            "block_s_max": float(d.max()), "sweeps_per_s": save_every / med,
            "chain_sweeps_per_s": save_every * nchains / med}


def run_bare(gb, x0, niter, save_every):
    import torch
    eng = gb._new_engine(x0)
    t = []
    t0 = time.perf_counter()
    for ii in range(niter):
        eng.sweep()
        if ii % save_every == 0 and ii > 0:
            torch.cuda.synchronize()
            t.append(time.perf_counter())
    torch.cuda.synchronize()
    return t, time.perf_counter() - t0


def run_sample(gb, x0, niter, save_every, outdir, **kw):
    clock = SavePointClock(sys.stdout)
    old = sys.stdout
    sys.stdout = clock
    t0 = time.perf_counter()
    try:
        gb.sample(x0, outdir=outdir, niter=niter, save_every=save_every, **kw)
    finally:
        sys.stdout = old
    return clock.t, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--kind", default="curn_red", choices=["curn", "curn_red", "curn_plred"])
    ap.add_argument("--n-psr", type=int, default=45)
    ap.add_argument("--nchains", type=int, default=2048)
    ap.add_argument("--niter", type=int, default=501)
    ap.add_argument("--save-every", type=int, default=100)
    ap.add_argument("--runs", default="bare,memory,disk8,disk8-device,diskall,diskall-device")
    ap.add_argument("--repeat", type=int, default=1, help="passes over the list of runs (alternating)")
    ap.add_argument("--workdir", default=None, help="where the chain directories go (default: a temporary one)")
    ap.add_argument("--out", default=None, help="JSON file for the results")
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("sample_rate needs a GPU: there is no CPU fallback")
    from pulsar_timing_gibbsspec_amd import PTABlockGibbs, synthetic
    redsample = "mh" if a.kind == "curn_plred" else "conditional"
    pta = synthetic.array_pta(kind=a.kind, n_psr=a.n_psr, seed=0)

    def new():
        return PTABlockGibbs(pta, hypersample="conditional", redsample=redsample, nchains=a.nchains, seed=1)
    np.random.seed(0)
    x0 = np.concatenate([np.atleast_1d(p.sample()).ravel() for p in new().params])
    work = a.workdir or tempfile.mkdtemp(prefix="sample_rate_")
    os.makedirs(work, exist_ok=True)
    results = []
    for rep in range(a.repeat):
        for name in a.runs.split(","):
            gb = new()
            outdir = os.path.join(work, f"{name}_{rep}")
            if name == "bare":
                t, wall = run_bare(gb, x0, a.niter, a.save_every)
            elif name == "memory":
                t, wall = run_sample(gb, x0, a.niter, a.save_every, outdir)
            elif name.startswith("disk"):
                spec, _, dest = name[4:].partition("-")
                if dest not in ("", "device"):
                    sys.exit(f"unknown run {name!r}")
                k = None if spec == "all" else int(spec)
                t, wall = run_sample(gb, x0, a.niter, a.save_every, outdir, history="disk", record_chains=k,
                                     slots=dest or "host")
            elif name.startswith("summary"):
                t, wall = run_sample(gb, x0, a.niter, a.save_every, outdir, history="summary",
                                     record_chains=int(name[7:] or 1))
            else:
                sys.exit(f"unknown run {name!r}")
            files = sum(os.path.getsize(os.path.join(outdir, f)) for f in os.listdir(outdir)) \
                if os.path.isdir(outdir) else 0
            res = {"run": name, "rep": rep, "kind": a.kind, "n_psr": a.n_psr, "nchains": a.nchains,
                   "niter": a.niter, "save_every": a.save_every, "npar": int(x0.size), "wall_s": wall,
                   "file_bytes": files, **block_stats(t, a.save_every, a.nchains)}
            print(json.dumps(res), flush=True)
            results.append(res)
            del gb
            shutil.rmtree(outdir, ignore_errors=True)
            torch.cuda.empty_cache()
    if a.workdir is None:
        shutil.rmtree(work, ignore_errors=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "workdir": work, "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
