"""What sample(history="summary", b_moments=True) of the single-pulsar samplers costs (MI355X).

    python tools/coef_moments_rate.py kernel    gs_coef_moments_block and gs_coef_moments_reduce alone
                                                on a fixed block, 1 x 4096 x 76 x 100, beside the
                                                derived floors: the block read once at the HBM rate and
                                                the 15 lower tiles' products at the FP64 roof
    python tools/coef_moments_rate.py block     per 100-sweep block of the configs[1] headline (J1713,
                                                4096 chains, save_every = 100), alternating in one
                                                process: C the summary mode without the keyword
                                                (tools/summary_block_rate.py's C: chain 0's b straight
                                                into the pinned slot), CW the same with every chain's b
                                                recorded into the HBM slot and chain 0 copied behind
                                                the block, CK that plus gs_coef_moments_block, CM the
                                                mode with the keyword (CK plus the save point's
                                                gs_coef_moments_reduce on the side stream and its
                                                three buffers).  CW - C: the sweep's extra b writes;
                                                CK - CW: the product kernel; CM - CK: the save point.

Each mode prints one JSON line.  Times are device events around --blocks timed blocks after a
warm-up of the same shape, best of --rounds."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.summary_block_rate import FP64_PEAK_TFLOPS, NF, S, event_ms  # noqa: E402

HBM_TBPS = 8.0                                     # the MI355X's HBM3E peak


def floors(C, m, ldb):
    nt = -(-m // 16)
    tiles = nt * (nt + 1) // 2
    flop = tiles * 16 * 16 * 2 * C * S
    nbytes = C * S * ldb * 8
    return dict(block_MB=round(nbytes / 1e6, 1), tiles=tiles, GFLOP=round(flop / 1e9, 2),
                read_floor_us=round(nbytes / (HBM_TBPS * 1e12) * 1e6, 1),
                mfma_floor_us=round(flop / (FP64_PEAK_TFLOPS * 1e12) * 1e6, 1))


def kernel(a):
    from pulsar_timing_gibbsspec_amd import _lib
    from pulsar_timing_gibbsspec_amd.engine import CoefMoments
    ctx = _lib.Context(0, seed=1)
    C, m = a.nchains, 76
    rng = np.random.default_rng(0)
    sd = 10.0 ** rng.uniform(-9, -3, m)
    b = torch.as_tensor(sd * 10.0 ** rng.uniform(0, 6, m) + sd * rng.standard_normal((S, C, m))).to(ctx.device)
    mom = CoefMoments(ctx, C, [m], m)
    bufs = [torch.zeros(s, dtype=torch.float64, device=ctx.device) for s in mom.extra_shapes]
    mom.accumulate_block(b, 0, S)
    mom.pack(*bufs)
    t_blk = [event_ms(ctx.stream, lambda: mom.accumulate_block(b, 0, S), a.blocks) for _ in range(a.rounds)]
    t_red = [event_ms(ctx.stream, lambda: mom.pack(*bufs), a.blocks) for _ in range(a.rounds)]
    f = floors(C, m, m)
    state_MB = mom.state.numel() * 8 / 1e6
    print(json.dumps(dict(mode="kernel", nchains=C, blocks=a.blocks, block_us=[round(v * 1e3, 1) for v in t_blk],
                          reduce_us=[round(v * 1e3, 1) for v in t_red], state_MB=round(state_MB, 1),
                          read_TBps=round(C * S * m * 8 / min(t_blk) / 1e9, 3),
                          TFLOPS=round(f["GFLOP"] / min(t_blk), 2), **f)), flush=True)


def block(a):
    from pulsar_timing_gibbsspec_amd import _lib, synthetic
    from pulsar_timing_gibbsspec_amd.engine import (ChainSummary, CoefMoments, DeviceModel, FreeSpectrumChains,
                                                    HistoryStreamer)
    C = a.nchains
    pta = synthetic.single_pulsar_pta("J1713+0747", seed=0)
    T, N, r = pta.get_basis()[0], pta.get_ndiag({})[0], pta.get_residuals()[0]
    ctx = _lib.Context(0, seed=1)
    model = DeviceModel(ctx, [T], [N], [r], [np.arange(2 * NF)], [np.full(T.shape[1] - 2 * NF, 1e-40)])
    x0 = np.random.default_rng(0).uniform(-9, -4, (C, NF))
    run = FreeSpectrumChains(model, 1e-18, 1e-8, C, x0)
    ldb, m = model.ldb, int(model.m[0])
    lo, hi = np.full(NF, -9.0), np.full(NF, -4.0)
    # one summary per leg: a save point's pack_behind makes the next accumulation wait for it
    summ = {k: ChainSummary(ctx, C, NF, lo, hi, n_bins=a.bins) for k in ("C", "CW", "CK", "CM")}
    mom = {k: CoefMoments(ctx, C, [m], ldb) for k in ("CK", "CM")}
    sx = [(1,) + tuple(e) for e in summ["C"].extra_shapes]
    mx = [(1,) + tuple(e) for e in mom["CM"].extra_shapes]
    keep = lambda t: t[:, :1]                      # noqa: E731
    # C: sample_free_spectrum's slots without the keyword; CW, CK: every chain's b in the HBM slot
    # and chain 0 of it sent; CM: also the moments' three buffers
    st = dict(C=HistoryStreamer(ctx, [(S, C, NF), (S, 1, ldb)] + sx, views=[keep, None, None, None],
                                direct=[False, True, False, False]))
    st["CW"] = HistoryStreamer(ctx, [(S, C, NF), (S, C, ldb)] + sx, views=[keep, keep, None, None])
    st["CK"] = st["CW"]
    st["CM"] = HistoryStreamer(ctx, [(S, C, NF), (S, C, ldb)] + sx + mx, views=[keep, keep] + [None] * 5)
    state = {"slot": 0, "pending": None}

    def leg(k):
        bk = 1 if k == "C" else C

        def fn():
            slot = state["slot"]
            xs, bs, *extra = st[k].buffers(slot, S)
            run.run(S, x_rec=xs, b_rec=bs, record_b_chains=bk)
            summ[k].accumulate_block(xs, run.it - S, S)
            if k in mom:
                mom[k].accumulate_block(bs, run.it - S, S)
            summ[k].pack_behind(st[k].side, extra[0][0], extra[1][0])
            if k == "CM":
                mom[k].pack_behind(st[k].side, *[e[0] for e in extra[2:]])
            st[k].submit(slot, S)
            if state["pending"] is not None:
                st[k].fetch(state["pending"])
            state["pending"], state["slot"] = slot, slot ^ 1
        return fn
    legs = [(k, leg(k)) for k in ("C", "CW", "CK", "CM")]
    t = {k: [] for k, _ in legs}
    for _, fn in legs:
        state["pending"] = None
        fn(), fn()                                 # warm every shape the timed window uses
    for _ in range(a.rounds):                      # alternate the legs
        for k, fn in legs:
            state["pending"] = None
            t[k].append(event_ms(ctx.stream, fn, a.blocks))
    best = {k: min(v) for k, v in t.items()}
    print(json.dumps(dict(mode="block", nchains=C, blocks=a.blocks, bins=a.bins, m=m, ldb=ldb,
                          ms={k: [round(x, 4) for x in v] for k, v in t.items()},
                          b_writes_us=round((best["CW"] - best["C"]) * 1e3, 1),
                          kernel_us=round((best["CK"] - best["CW"]) * 1e3, 1),
                          save_point_us=round((best["CM"] - best["CK"]) * 1e3, 1),
                          CM_minus_C_us=round((best["CM"] - best["C"]) * 1e3, 1),
                          C_spread_us=round((max(t["C"]) - min(t["C"])) * 1e3, 1),
                          **floors(C, m, ldb))), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("mode", choices=("kernel", "block"))
    p.add_argument("--blocks", type=int, default=50)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--bins", type=int, default=64)
    p.add_argument("--nchains", type=int, default=4096)
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("coef_moments_rate.py measures on the GPU: none is visible")
    {"kernel": kernel, "block": block}[a.mode](a)


if __name__ == "__main__":
    main()
