"""chain_writer.ChainWriter (CPU): the streamed files of PTABlockGibbs.sample(history="disk")
hold what was appended, in bounded host memory, and reopen for a resume."""
import io
import os
import tracemalloc

import numpy as np
import pytest

from pulsar_timing_gibbsspec_amd.chain_writer import ChainWriter

K, ROWS, NPAR, NBLK = 64, 100, 50, 20


@pytest.fixture(scope="module")
def blocks():
    rng = np.random.default_rng(5)
    b = [rng.standard_normal((K, ROWS, NPAR)) for _ in range(NBLK)]
    for a in b:
        a.setflags(write=False)
    return b


def _savetxt_bytes(rows):
    f = io.BytesIO()
    np.savetxt(f, rows)
    return f.getvalue()


def _check_files(d, blocks):
    full = np.concatenate(blocks, axis=1)
    assert np.array_equal(np.load(os.path.join(d, "chains.npy")), full)
    assert open(os.path.join(d, "chain.txt"), "rb").read() == _savetxt_bytes(full[0])
    st = np.load(os.path.join(d, "gibbs_state.npz"))
    assert int(st["rows"]) == full.shape[1] and int(st["thin"]) == 1 and int(st["record_chains"]) == K


def test_content(tmp_path, blocks):
    w = ChainWriter(tmp_path, K, NBLK * ROWS, NPAR)
    for i, b in enumerate(blocks):
        w.append(b)
        assert w.rows_written == (i + 1) * ROWS
    w.close()
    _check_files(tmp_path, blocks)


def _peak_over_appends(append, blocks):
    tracemalloc.start()
    try:
        base = tracemalloc.get_traced_memory()[0]
        tracemalloc.reset_peak()
        for b in blocks:                       # made before tracing started
            append(b)
        return tracemalloc.get_traced_memory()[1] - base
    finally:
        tracemalloc.stop()


def test_memory_is_bounded(tmp_path, blocks):
    """The peak traced allocation over the 20 appends stays below a quarter of the bytes appended:
    a writer that retains the history fails, one that holds a few blocks passes."""
    total = sum(b.nbytes for b in blocks)
    w = ChainWriter(tmp_path / "w", K, NBLK * ROWS, NPAR)
    peak = _peak_over_appends(w.append, blocks)
    w.close()
    print(f"appended {total} bytes, peak traced {peak} bytes")
    assert peak < total / 4
    _check_files(tmp_path / "w", blocks)


def test_memory_probe_is_sound(tmp_path, blocks):
    """The measurement itself: a plain per-block memmap assignment stays inside the bound, a
    writer that keeps every block does not."""
    total = sum(b.nbytes for b in blocks)
    mm = np.lib.format.open_memmap(tmp_path / "plain.npy", mode="w+", dtype=np.float64,
                                   shape=(K, NBLK * ROWS, NPAR))
    at = [0]

    def plain(b):
        mm[:, at[0]:at[0] + b.shape[1]] = b
        at[0] += b.shape[1]
    assert _peak_over_appends(plain, blocks) < total / 4
    kept = []
    assert _peak_over_appends(lambda b: kept.append(b.copy()), blocks) >= total / 4


def test_uncommitted_rows_wait_for_the_next_commit(tmp_path, blocks):
    w = ChainWriter(tmp_path, K, 2 * ROWS, NPAR)
    w.append(blocks[0], commit=False)
    assert w.rows_written == 0 and os.path.getsize(tmp_path / "chain.txt") == 0
    assert not os.path.exists(tmp_path / "gibbs_state.npz")
    w.append(blocks[1], state={"x": np.arange(3.0)})
    assert w.rows_written == 2 * ROWS
    _check_files(tmp_path, blocks[:2])
    assert np.array_equal(np.load(tmp_path / "gibbs_state.npz")["x"], np.arange(3.0))


def test_thinned_state_rows(tmp_path, blocks):
    """With thin = t the state counts sweeps: rows -> ceil(rows / t) file rows; a state that does
    not describe the rows written is refused."""
    w = ChainWriter(tmp_path, K, 2 * ROWS, NPAR, thin=5)
    w.append(blocks[0], state={"rows": 5 * ROWS - 4})
    with pytest.raises(ValueError):
        w.append(blocks[1], state={"rows": 5 * ROWS})
    r = ChainWriter(tmp_path, K, 2 * ROWS, NPAR, thin=5, resume=True)
    assert r.rows_written == ROWS
    with pytest.raises(ValueError):
        ChainWriter(tmp_path, K, 2 * ROWS, NPAR, thin=1, resume=True)


def test_reopen_for_resume(tmp_path, blocks):
    w = ChainWriter(tmp_path, K, NBLK * ROWS, NPAR)
    for b in blocks[:7]:
        w.append(b)
    w.append(blocks[7], commit=False)            # rows the state file does not describe: dropped
    w.close()
    del w
    r = ChainWriter(tmp_path, K, NBLK * ROWS, NPAR, resume=True)
    assert r.rows_written == 7 * ROWS and int(r.state["rows"]) == 7 * ROWS
    for b in blocks[7:]:
        r.append(b)
    r.close()
    _check_files(tmp_path, blocks)


def test_reopen_resizes_for_another_length(tmp_path, blocks):
    w = ChainWriter(tmp_path, K, 3 * ROWS, NPAR)
    for b in blocks[:2]:
        w.append(b)
    w.close()
    del w
    r = ChainWriter(tmp_path, K, 5 * ROWS, NPAR, resume=True)
    assert r.chains.shape == (K, 5 * ROWS, NPAR) and r.rows_written == 2 * ROWS
    for b in blocks[2:5]:
        r.append(b)
    r.close()
    _check_files(tmp_path, blocks[:5])


def test_reopen_with_wrong_shape_raises(tmp_path, blocks):
    w = ChainWriter(tmp_path, K, 3 * ROWS, NPAR)
    w.append(blocks[0])
    w.close()
    del w
    for shape in ((K - 1, 3 * ROWS, NPAR), (K, 3 * ROWS, NPAR + 1), (K, ROWS - 1, NPAR)):
        with pytest.raises(ValueError, match="cannot resume"):
            ChainWriter(tmp_path, *shape, resume=True)
    with pytest.raises(ValueError, match="cannot resume"):
        ChainWriter(tmp_path / "empty", K, ROWS, NPAR, resume=True)
    with pytest.raises(ValueError):
        ChainWriter(tmp_path, K, 3 * ROWS, NPAR, resume=True).append(blocks[0][:, :, :-1])
