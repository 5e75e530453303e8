"""What the CPU tests of the stream drivers share to run batch_stream on the oracle backend: the residual query replaced by a
function of the window alone, MargHandle.compute_batch and VioLib.batch_solve over the oracle's contexts, and a recording handle
that keeps every batched call's arguments."""
import numpy as np

import fm_stream_reference as fsr


def stub_flags(w):
    """The residual query's flags as a function of the window alone: bit 0 (outlier) for every seventh landmark index, bit 1 (behind a
    camera) for every eleventh."""
    n = int(w.n_landmarks)
    f = np.zeros(n, dtype=np.uint8)
    f[3::7] |= 1
    f[5::11] |= 2
    return f


def stub_driver(d):
    d.ctx.residuals = lambda w, focal=None, outlier_px=3.0: dict(flags=stub_flags(w))
    return d


class OracleMarg:
    """MargHandle.compute_batch on the CPU backend: each job through a context's load + marginalize."""

    def __init__(self, lib):
        self.lib = lib

    def compute_batch(self, jobs):
        out = []
        for kind, w, prior in jobs:
            assert w.prior is prior
            c = self.lib.context()
            c.load(w)
            out.append(c.marginalize(kind))
        return out


def patch_batched(monkeypatch, oracle_lib):
    """batch_solve and batch_residuals (stub_flags) on the oracle library; returns the list the residual calls are noted in as
    (windows, threshold, outputs)."""
    seen = []

    def batch_residuals(ctxs, windows, focal=None, outlier_px=3.0, outputs=None):
        seen.append((len(ctxs), outlier_px, outputs))
        return [dict(flags=stub_flags(w)) for w in windows]
    monkeypatch.setattr(oracle_lib, "batch_solve", lambda ctxs, iterations=10: [c.solve(iterations) for c in ctxs], raising=False)
    monkeypatch.setattr(oracle_lib, "batch_residuals", batch_residuals, raising=False)
    return seen


def frozen(v):
    """A call argument as a value that compares by content: arrays by dtype, shape and bytes, floats by their bits."""
    if isinstance(v, np.ndarray):
        return ("array", str(v.dtype), v.shape, v.tobytes())
    if isinstance(v, (list, tuple)):
        return tuple(frozen(x) for x in v)
    if isinstance(v, dict):
        return tuple((k, frozen(x)) for k, x in sorted(v.items()))
    if isinstance(v, (float, np.floating)):
        return ("float", float(v).hex())
    if isinstance(v, (bool, np.bool_)):
        return bool(v)
    if isinstance(v, (int, np.integer)):
        return int(v)
    return v


class ArgRecording(fsr.Recording):
    """fsr.Recording that also keeps, in `args`, (method, items, further arguments) of every batched call, frozen."""

    def __init__(self, handle):
        fsr.Recording.__init__(self, handle)
        self.args = []

    def __getattr__(self, name):
        call = fsr.Recording.__getattr__(self, name)
        if not name.endswith("_batch"):
            return call

        def recorded(items, *a, **kw):
            self.args.append((name, frozen(items), frozen(a), frozen(kw)))
            return call(items, *a, **kw)
        return recorded
