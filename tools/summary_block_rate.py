"""What sample(history="summary") of the single-pulsar samplers costs (MI355X).

    python tools/summary_block_rate.py kernel     gs_chain_summary_block against gs_chain_summary on
                                                  fixed data: 1 x 4096 x 30 x 100 (one call of the old
                                                  entry) and 45 x 256 x 30 x 100 (45 calls)
    python tools/summary_block_rate.py block      per 100-sweep block of the configs[1] headline
                                                  (J1713, 4096 chains): A the fused sweep recording x
                                                  into HBM only, B the default sample() stream (x rows
                                                  and chain 0's b written to pinned host memory),
                                                  C the summary mode as sample(save_every=100) queues
                                                  it (x into an HBM slot, the summary kernel, the save
                                                  point's finalize / pack into the slot's two extra
                                                  buffers on the side stream, chain 0's x and the
                                                  extras copied behind the block), C0 the same without
                                                  finalize / pack; with --acf-lags L also CL, C with
                                                  acf_lags=L (gs_chain_acf_block behind the summary
                                                  kernel, gs_chain_acf_reduce and acov in a third
                                                  extra buffer), beside the kernel's FMA floor at the
                                                  FP64 vector roof bench.py uses
    python tools/summary_block_rate.py sample --history memory|summary [--nchains N --niter N]
                                                  PulsarBlockGibbs.sample end to end in this process:
                                                  wall time, chain-it/s and peak host memory (ru_maxrss)

Each mode prints one JSON line.  Times are device events around at least --blocks timed blocks
after a warm-up of the same shape; A, B and C alternate in one process."""
import argparse
import json
import os
import resource
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NF, S = 30, 100
FP64_PEAK_TFLOPS = 78.6                            # bench.py's FP64 vector roof of the MI355X


def event_ms(stream, fn, n):
    """Mean ms of fn() over n calls, device events on the stream around all of them."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record(stream)
    for _ in range(n):
        fn()
    t1.record(stream)
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / n


def kernel(a):
    from pulsar_timing_gibbsspec_amd import _lib
    from pulsar_timing_gibbsspec_amd._lib import check, ptr
    from pulsar_timing_gibbsspec_amd.engine import ChainSummary
    ctx = _lib.Context(0, seed=1)
    lo, hi = np.full(NF, -9.0), np.full(NF, -4.0)
    out = {"mode": "kernel", "blocks": a.blocks, "bins": a.bins}
    for G, C in ((1, 4096), (45, 256)):
        # a posterior-like block: each parameter's values cluster, as recorded chains do
        rng = np.random.default_rng(G)
        centre = rng.uniform(-8.0, -5.0, NF)
        x = torch.as_tensor(centre + 0.3 * rng.standard_normal((S, G * C, NF))).to(ctx.device)
        new = ChainSummary(ctx, C, NF, lo, hi, n_bins=a.bins, n_group=G)
        old = ChainSummary(ctx, C, NF, lo, hi, n_bins=a.bins, n_group=G)
        oc, oo = old.counts.view(G, NF, a.bins), old.outside.view(G, NF)

        def run_new():
            new.accumulate_block(x, 0, S)

        def run_old():
            for g in range(G):
                rows = slice(g * C, (g + 1) * C)
                check(ctx.lib.gs_chain_summary(
                    ctx.handle, C, NF, ptr(x.view(-1)[g * C * NF:]), S, G * C * NF, 0, 0, a.bins, ptr(old.lo),
                    ptr(old.hi), ptr(old.scale), ptr(old.mid), ptr(old.s1[rows]), ptr(old.s2[rows]), ptr(oc[g]),
                    ptr(oo[g]), ptr(old.n_acc)), "gs_chain_summary")
        run_new(), run_old()
        torch.cuda.synchronize()
        same = bool(torch.equal(new.counts.view(-1), old.counts.view(-1)) and torch.equal(new.s1, old.s1))
        t = {"new": [], "old": []}
        for _ in range(3):                         # alternate the two, three rounds each
            t["new"].append(event_ms(ctx.stream, run_new, a.blocks))
            t["old"].append(event_ms(ctx.stream, run_old, a.blocks))
        nbytes = x.numel() * 8 + 4 * new.s1.numel() * 8    # the block read, s1 and s2 read and written
        out[f"{G}x{C}"] = dict(new_us=[round(v * 1e3, 2) for v in t["new"]], old_us=[round(v * 1e3, 2) for v in t["old"]],
                               bytes=nbytes, new_TBps=round(nbytes / min(t["new"]) / 1e9, 3), equal=same)
    print(json.dumps(out), flush=True)


def block(a):
    from pulsar_timing_gibbsspec_amd import _lib, synthetic
    from pulsar_timing_gibbsspec_amd.engine import ChainSummary, DeviceModel, FreeSpectrumChains, HistoryStreamer
    C = a.nchains
    pta = synthetic.single_pulsar_pta("J1713+0747", seed=0)
    T, N, r = pta.get_basis()[0], pta.get_ndiag({})[0], pta.get_residuals()[0]
    ctx = _lib.Context(0, seed=1)
    model = DeviceModel(ctx, [T], [N], [r], [np.arange(2 * NF)], [np.full(T.shape[1] - 2 * NF, 1e-40)])
    x0 = np.random.default_rng(0).uniform(-9, -4, (C, NF))
    run = FreeSpectrumChains(model, 1e-18, 1e-8, C, x0)
    dev = ctx.device
    xr = torch.empty(S, C, NF, dtype=torch.float64, device=dev)
    br = torch.empty(S, 1, model.ldb, dtype=torch.float64, device=dev)
    # B: what sample() does by default -- x rows and chain 0's b straight into pinned slots
    direct = HistoryStreamer(ctx, [(S, C, NF), (S, 1, model.ldb)], direct=[True, True])
    # C: the summary mode as sample_free_spectrum builds it -- x into HBM slots, chain 0 copied
    # behind the block, b as in B, and every block a save point (save_every = 100): finalize / pack
    # into two extra buffers of the slot.  C0: the same without the save point's finalize / pack.
    summ = ChainSummary(ctx, C, NF, np.full(NF, -9.0), np.full(NF, -4.0), n_bins=a.bins)
    shapes, keep = [(S, C, NF), (S, 1, model.ldb)], (lambda t: t[:, :1])
    hbm0 = HistoryStreamer(ctx, shapes, views=[keep, None], direct=[False, True])
    hbm = HistoryStreamer(ctx, shapes + [(1,) + tuple(e) for e in summ.extra_shapes],
                          views=[keep, None, None, None], direct=[False, True, False, False])
    state = {"slot": 0, "pending": None}

    def run_a():
        run.run(S, x_rec=xr, b_rec=br, record_b_chains=1)

    def streamed(st, after=None):
        slot = state["slot"]
        xs, bs, *extra = st.buffers(slot, S)
        run.run(S, x_rec=xs, b_rec=bs, record_b_chains=1)
        if after is not None:
            after(xs, extra)
        st.submit(slot, S)
        if state["pending"] is not None:
            st.fetch(state["pending"])
        state["pending"], state["slot"] = slot, slot ^ 1

    def run_b():
        streamed(direct)

    def run_c0():
        streamed(hbm0, lambda xs, extra: summ.accumulate_block(xs, run.it - S, S))

    def run_c():
        def after(xs, extra):
            summ.accumulate_block(xs, run.it - S, S)
            summ.pack_behind(hbm.side, extra[0][0], extra[1][0])
        streamed(hbm, after)
    legs = [("A", run_a), ("B", run_b), ("C0", run_c0), ("C", run_c)]
    acf = {}
    if a.acf_lags:
        # CL: C with acf_lags -- its own summary (the ACF state) and a slot with the third buffer
        summ_l = ChainSummary(ctx, C, NF, np.full(NF, -9.0), np.full(NF, -4.0), n_bins=a.bins, acf_lags=a.acf_lags)
        hbm_l = HistoryStreamer(ctx, shapes + [(1,) + tuple(e) for e in summ_l.extra_shapes],
                                views=[keep, None, None, None, None], direct=[False, True, False, False, False])

        def run_cl():
            def after(xs, extra):
                summ_l.accumulate_block(xs, run.it - S, S)
                summ_l.pack_behind(hbm_l.side, *[e[0] for e in extra])
            streamed(hbm_l, after)
        legs.append(("CL", run_cl))
    t = {k: [] for k, _ in legs}
    for _, fn in legs:
        state["pending"] = None
        fn(), fn()                                 # warm every shape the timed window uses
    for _ in range(a.rounds):                      # alternate the legs
        for k, fn in legs:
            state["pending"] = None
            t[k].append(event_ms(ctx.stream, fn, a.blocks))
    best = {k: min(v) for k, v in t.items()}
    if a.acf_lags:
        fma = C * NF * S * (a.acf_lags + 1)        # (L + 1) per recorded value
        acf = dict(acf_lags=a.acf_lags, CL_minus_C_us=round((best["CL"] - best["C"]) * 1e3, 1),
                   C_spread_us=round((max(t["C"]) - min(t["C"])) * 1e3, 1), acf_fma=fma,
                   acf_fma_floor_us=round(fma / (FP64_PEAK_TFLOPS / 2 * 1e12) * 1e6, 1),
                   acf_state_MB=round(summ_l.acf_state.numel() * 8 / 1e6, 1))
    print(json.dumps(dict(mode="block", nchains=C, blocks=a.blocks, bins=a.bins, **acf,
                          ms={k: [round(x, 4) for x in v] for k, v in t.items()},
                          C_minus_A_us=round((best["C"] - best["A"]) * 1e3, 1),
                          C0_minus_A_us=round((best["C0"] - best["A"]) * 1e3, 1),
                          B_minus_A_us=round((best["B"] - best["A"]) * 1e3, 1),
                          chain_it_per_s={k: round(C * S / (v * 1e-3), 0) for k, v in best.items()})), flush=True)


def sample(a):
    from pulsar_timing_gibbsspec_amd import PulsarBlockGibbs, synthetic
    pta = synthetic.single_pulsar_pta("J1713+0747", seed=0)
    gb = PulsarBlockGibbs(pta, nchains=a.nchains, seed=1)
    x0 = np.random.default_rng(0).uniform(-9, -4, NF)
    kw = dict(history="summary", bins=a.bins) if a.history == "summary" else {}
    if a.acf_lags:
        kw["acf_lags"] = a.acf_lags
    with tempfile.TemporaryDirectory() as d:
        gb.sample(x0, outdir=d, niter=1 + S, **kw)                       # warm-up: code objects, pinned slots
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gb.sample(x0, outdir=d, niter=a.niter, **kw)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    print(json.dumps(dict(mode="sample", history=a.history, nchains=a.nchains, niter=a.niter, wall_s=round(wall, 3),
                          chain_it_per_s=round(a.nchains * a.niter / wall, 0),
                          maxrss_MB=round(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024, 1))), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("mode", choices=("kernel", "block", "sample"))
    p.add_argument("--blocks", type=int, default=50)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--bins", type=int, default=64)
    p.add_argument("--nchains", type=int, default=4096)
    p.add_argument("--niter", type=int, default=5001)
    p.add_argument("--history", choices=("memory", "summary"), default="summary")
    p.add_argument("--acf-lags", type=int, default=0, help="block: also time C with acf_lags=L; sample: pass it on")
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("summary_block_rate.py measures on the GPU: none is visible")
    {"kernel": kernel, "block": block, "sample": sample}[a.mode](a)


if __name__ == "__main__":
    main()
