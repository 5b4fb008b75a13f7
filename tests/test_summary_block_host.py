"""gs_chain_summary_block and the history keyword of the single-pulsar samplers, as far as they go
without a device (CPU only)."""
import numpy as np
import pytest


def test_block_entry_rejects_a_null_context():
    from pulsar_timing_gibbsspec_amd import _lib
    L = _lib.load()
    rc = L.gs_chain_summary_block(None, 1, 1, 1, None, 1, 1, 0, 0, 1, None, None, None, None, None, None, None,
                                  None, None)
    assert rc == 1
    assert b"ctx" in L.gs_last_error()


def test_unknown_history_is_rejected_before_anything_is_touched(tmp_path):
    from pulsar_timing_gibbsspec_amd import PulsarBlockGibbs, synthetic
    gb = PulsarBlockGibbs(synthetic.single_pulsar_pta("J1713+0747", seed=0), nchains=2, seed=5)
    d = tmp_path / "never"
    with pytest.raises(ValueError):
        gb.sample(np.full(30, -6.0), outdir=str(d), niter=10, history="nope")
    with pytest.raises(ValueError):
        gb.sample(np.full(30, -6.0), outdir=str(d), niter=10, bins=64)     # given without history="summary"
    assert not d.exists() and gb._ctx is None      # no directory, no device context
