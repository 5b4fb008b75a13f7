"""``ChainWriter`` -- the files of a streamed ``PTABlockGibbs.sample(history="disk")`` run.

Pure numpy, importable without a GPU.  The writer owns three files of a chain directory:

``chains.npy``       a memory map (``np.lib.format.open_memmap``) of shape (nchains, nrows, npar),
                     chain-major, created once at its final size and filled block by block.
                     Rows at and beyond ``rows_written`` are UNWRITTEN (zeros of a sparse file, or
                     rows of a block that was never committed): read ``[:, :rows_written]`` only.
``chain.txt``        chain 0's rows in ``np.savetxt``'s default format, extended by append, so its
                     bytes equal one ``np.savetxt`` of all the rows written so far.
``gibbs_state.npz``  what a resume needs; (re)written only after the rows it describes are in the
                     two files above.  ``rows`` counts sweeps: with ``thin`` = t the files hold
                     the ceil(rows / t) rows of the sweeps ii < rows with ii % t == 0.

Host memory: nothing is kept between appends but the open map; an append formats chain 0's new
rows only.
"""
from __future__ import annotations

import os

import numpy as np

STATE = "gibbs_state.npz"


def _count_lines(path):
    n = 0
    with open(path, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 20), b""):
            n += chunk.count(b"\n")
    return n


def _truncate_lines(path, nlines):
    """Keep the first nlines lines of a text file (in place, reading 1 MiB at a time)."""
    pos = seen = 0
    with open(path, "rb+") as f:
        while seen < nlines:
            chunk = f.read(1 << 20)
            if not chunk:
                raise ValueError(f"{path} holds {seen} rows, the state file describes {nlines}")
            at = -1
            while seen < nlines:
                at = chunk.find(b"\n", at + 1)
                if at < 0:
                    break
                seen += 1
            pos += len(chunk) if seen < nlines else at + 1
        f.truncate(pos)


class ChainWriter:
    """Append-only writer of chains.npy / chain.txt / gibbs_state.npz (see the module docstring).

    ChainWriter(outdir, nchains, nrows, npar)               a new run: files are created / emptied
    ChainWriter(..., resume=True)                           reopen: continue after the rows the state
                                                            file describes (the map is resized if nrows
                                                            changed); raises ValueError on a mismatch
    ChainWriter(..., adopt=rows0)                           a new map whose chain 0 starts with the
                                                            rows of an existing chain.txt (kept as is)
    """

    def __init__(self, outdir, nchains, nrows, npar, *, thin=1, resume=False, adopt=None):
        self.outdir = str(outdir)
        self.K, self.nrows, self.npar, self.thin = int(nchains), int(nrows), int(npar), int(thin)
        if self.K <= 0 or self.nrows < 0 or self.npar <= 0 or self.thin <= 0:
            raise ValueError("nchains, npar and thin must be positive, nrows non-negative")
        os.makedirs(self.outdir, exist_ok=True)
        self.npy = os.path.join(self.outdir, "chains.npy")
        self.txt = os.path.join(self.outdir, "chain.txt")
        self.state_file = os.path.join(self.outdir, STATE)
        self.state = None            # the state file's content at reopen
        self._pending = []           # chain 0's rows of uncommitted appends
        self._filled = 0             # rows in the map, committed or not
        shape = (self.K, self.nrows, self.npar)
        if resume:
            self._reopen(shape)
            return
        self.chains = np.lib.format.open_memmap(self.npy, mode="w+", dtype=np.float64, shape=shape)
        self.rows_written = 0
        if adopt is not None:
            adopt = np.atleast_2d(np.asarray(adopt, float))
            if adopt.shape[1] != self.npar or adopt.shape[0] > self.nrows or self.thin != 1:
                raise ValueError("adopted rows need thin=1, npar columns and at most nrows rows")
            self.chains[0, :adopt.shape[0]] = adopt
            self.rows_written = adopt.shape[0]
        else:
            open(self.txt, "wb").close()
        if os.path.exists(self.state_file):
            os.remove(self.state_file)           # it described the files this run replaces
        self._filled = self.rows_written

    # ------------------------------------------------------------ resume
    def _reopen(self, shape):
        if not os.path.exists(self.state_file):
            raise ValueError(f"cannot resume: {self.state_file} is missing")
        with np.load(self.state_file, allow_pickle=False) as st:
            self.state = {k: st[k] for k in st.files}
        thin = int(self.state.get("thin", 1))
        if thin != self.thin:
            raise ValueError(f"cannot resume: the run was recorded with thin={thin}, not thin={self.thin}")
        n = -(-int(self.state["rows"]) // self.thin)
        if not os.path.exists(self.npy):
            raise ValueError(f"cannot resume: {self.npy} is missing")
        old = np.lib.format.open_memmap(self.npy, mode="r+")
        if old.ndim != 3 or old.dtype != np.float64 or (old.shape[0], old.shape[2]) != (shape[0], shape[2]) \
                or old.shape[1] < n:
            raise ValueError(f"cannot resume: {self.npy} has shape {old.shape} {old.dtype}, this run records "
                             f"(chains, rows, parameters) = {shape} and the state file describes {n} rows")
        if n > shape[1]:
            raise ValueError(f"cannot resume: {n} rows are on disk, this run keeps only {shape[1]}")
        if old.shape[1] != shape[1]:
            # another niter: a map of the new size, the written rows copied a few chains at a time
            tmp = self.npy + ".resize.npy"
            new = np.lib.format.open_memmap(tmp, mode="w+", dtype=np.float64, shape=shape)
            step = max(1, (1 << 26) // max(1, 8 * n * shape[2]))
            for c in range(0, shape[0], step):
                new[c:c + step, :n] = old[c:c + step, :n]
            new.flush()
            del new, old
            os.replace(tmp, self.npy)
            old = np.lib.format.open_memmap(self.npy, mode="r+")
        self.chains = old
        if not os.path.exists(self.txt) or _count_lines(self.txt) < n:
            raise ValueError(f"cannot resume: {self.txt} holds fewer than the {n} rows of the state file")
        _truncate_lines(self.txt, n)             # rows appended after the last state file was written
        self.rows_written = self._filled = n

    # ------------------------------------------------------------ append
    def append(self, block, state=None, commit=True):
        """Write block [nchains, rows, npar] after the rows already in the map.  commit=True also
        appends chain 0's rows to chain.txt and then rewrites the state file: ``rows`` (sweeps
        done; default: the sweep after the last row), ``thin``, ``record_chains`` and the arrays of
        ``state``.  commit=False only fills the map (chain 0's rows wait in memory for the next
        commit): until then the rows count as unwritten."""
        block = np.asarray(block)
        if block.ndim != 3 or block.shape[0] != self.K or block.shape[2] != self.npar:
            raise ValueError(f"block of shape {block.shape}, expected ({self.K}, rows, {self.npar})")
        r0, r1 = self._filled, self._filled + block.shape[1]
        if r1 > self.nrows:
            raise ValueError(f"{r1} rows appended to a history of {self.nrows}")
        self.chains[:, r0:r1] = block
        self._pending.append(np.array(block[0], dtype=np.float64))
        self._filled = r1
        if not commit:
            return
        self.chains.flush()
        with open(self.txt, "ab") as f:
            for rows in self._pending:
                np.savetxt(f, rows)
            f.flush()
            os.fsync(f.fileno())
        self._pending = []
        self.rows_written = r1
        st = dict(state or {})
        st.setdefault("rows", (r1 - 1) * self.thin + 1 if r1 else 0)
        if -(-int(st["rows"]) // self.thin) != r1:
            raise ValueError(f"state rows={int(st['rows'])} (thin={self.thin}) does not describe the {r1} rows written")
        st["thin"], st["record_chains"] = self.thin, self.K
        tmp = os.path.join(self.outdir, "gibbs_state.tmp.npz")
        np.savez(tmp, **st)
        os.replace(tmp, self.state_file)

    def close(self):
        if getattr(self, "chains", None) is not None:
            self.chains.flush()
