"""gs_pta_record_block alone: the chain-major block record whose destination slot is selected
on the device (include/pulsar_gibbs.h)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = 4


def _run(C, npar, n_rec, pinned):
    from pulsar_timing_gibbsspec_amd import _lib
    ctx = _lib.Context(0, seed=1)
    dev = ctx.device
    stride, row_off = ROWS * npar, 2 * npar
    n_slot = max(n_rec, 1) * stride
    if pinned:
        slot = [torch.full((n_slot,), float("nan"), dtype=torch.float64, pin_memory=True) for _ in range(2)]
    else:
        slot = [torch.full((n_slot,), float("nan"), dtype=torch.float64, device=dev) for _ in range(2)]
    table = torch.tensor([s.data_ptr() for s in slot], dtype=torch.int64, device=dev)
    sel = torch.zeros(1, dtype=torch.int32, device=dev)
    g = torch.Generator().manual_seed(C * 1000 + npar)
    xs = [torch.rand(C, npar, dtype=torch.float64, generator=g).to(dev) for _ in range(2)]
    xlast = [torch.full((C,), float("nan"), dtype=torch.float64, device=dev) for _ in range(2)]
    for s in (0, 1):
        sel.fill_(s)
        _lib.check(ctx.lib.gs_pta_record_block(ctx.handle, C, npar, _lib.ptr(xs[s]), n_rec, stride, row_off,
                                               _lib.ptr(table), _lib.ptr(sel), _lib.ptr(xlast[s])),
                   "gs_pta_record_block")
    ctx.stream.synchronize()
    for s in (0, 1):
        got = slot[s].view(max(n_rec, 1), ROWS, npar)[:n_rec].to(dev)
        assert torch.equal(got[:, 2], xs[s][:n_rec])                      # the targeted elements, exactly
        rest = torch.ones(max(n_rec, 1), ROWS, npar, dtype=torch.bool)
        rest[:n_rec, 2] = False
        assert torch.isnan(slot[s].cpu().view(rest.shape)[rest]).all()    # nothing else was touched
        assert torch.equal(xlast[s], xs[s][:, -1])                        # for every chain, recorded or not


@pytest.mark.parametrize("C,npar,n_rec", [(5, 7, 3), (70, 129, 70), (3, 1, 0)])
def test_record_block_device_slots(C, npar, n_rec):
    """An odd npar, more chains than one wave covers and rows longer than one 512-byte run, a
    single column with nothing recorded (xlast only)."""
    _run(C, npar, n_rec, pinned=False)


def test_record_block_pinned_host_slots():
    """The slots in pinned host memory, written by the kernel and read after a stream sync."""
    _run(70, 129, 70, pinned=True)


def test_record_block_rejects_bad_arguments():
    from pulsar_timing_gibbsspec_amd import _lib
    ctx = _lib.Context(0, seed=1)
    dev = ctx.device
    x = torch.zeros(4, 3, dtype=torch.float64, device=dev)
    xl = torch.zeros(4, dtype=torch.float64, device=dev)
    buf = torch.zeros(4 * 12, dtype=torch.float64, device=dev)
    table = torch.tensor([buf.data_ptr()] * 2, dtype=torch.int64, device=dev)
    sel = torch.zeros(1, dtype=torch.int32, device=dev)
    p = _lib.ptr

    def rc(n_rec=4, stride=12, off=3, slots=table, s=sel):
        return ctx.lib.gs_pta_record_block(ctx.handle, 4, 3, p(x), n_rec, stride, off, p(slots), p(s), p(xl))
    assert rc() == 0
    assert rc(n_rec=5) != 0 and rc(n_rec=-1) != 0          # more rows than chains
    assert rc(stride=2) != 0                                # a row does not fit its chain's stride
    assert rc(off=10) != 0 and rc(off=-1) != 0              # the row would leave the chain's rows
    assert rc(slots=None) != 0 and rc(s=None) != 0
    assert rc(n_rec=0, slots=None, s=None) == 0             # xlast only needs no slot
    ctx.stream.synchronize()
    assert np.isfinite(buf.cpu().numpy()).all()
