"""The sampling entry points (csrc/sample.hip): pdn_sample_rows_f32 and pdn_decode_sample_tick_f32, launch counter 28.  Both
run the contract of pydynet_amd/llm/sampling.py on the fp32 rows; `margin` is the float64 distance of a draw from a decision
boundary (the GPU tests skip draws that close).
(One part of the TEST-ONLY host emulation of the pdnhip C ABI: see tests/abi_emulator/__init__.py.)"""
import numpy as np

from pydynet_amd.llm import sampling
from ._base import view, flat


def read_sample_params(ptr):
    """(temperature, top_k, top_p, seed) of the 24-byte sampling parameter block."""
    raw = np.array(flat(ptr, 3, np.int64)).view(np.uint8)
    return (float(raw[0:4].view(np.float32)[0]), int(raw[4:8].view(np.int32)[0]), float(raw[8:12].view(np.float32)[0]),
            int(raw[16:24].view(np.uint64)[0]))


def margin(z, t, b, temperature, top_k, top_p, seed):
    """float64 distance of row b's draw from the nearest decision boundary, relative to the total mass 1: the CDF steps
    against u, the top-p mass of the value groups against top_p, the top-k gap at the k-th value (relative to its size)."""
    z = np.asarray(z, np.float64)
    V = z.shape[0]
    out = np.inf
    if 0 < top_k < V:
        s = np.sort(z)[::-1]
        out = min(out, (s[top_k - 1] - s[top_k]) / max(1.0, abs(s[top_k - 1])) if s[top_k - 1] != s[top_k] else np.inf)
    if top_p < 1.0:
        kept = np.ones(V, bool) if not 0 < top_k < V else z >= np.partition(z, V - top_k)[V - top_k]
        w = np.where(kept, np.exp((z - z.max()) / temperature), 0.0)
        vals, grp = np.unique(z[kept], return_inverse=True)
        cum = np.cumsum(np.bincount(grp.reshape(-1), weights=(w / w.sum())[kept], minlength=vals.size)[::-1])
        out = min(out, float(np.abs(cum - top_p).min()))
    _, p = sampling.kept_mask(z, top_k, top_p, temperature)
    u = sampling.uniforms(t, [b], seed)[0]
    out = min(out, float(np.abs(np.cumsum(p)[p > 0] - u).min()))
    return out


class SamplingMixin:
    def _sample_rows(self, logits, rs, B, V, params, t, out):
        if B == 0:
            return 0
        T, k, p, seed = read_sample_params(params)
        z = np.array(view(logits, (B, V), (rs, 1), np.float32))
        flat(out, B, np.int64)[...] = sampling.sample_rows_np(z, int(t), T, k, p, seed) if T > 0 else z.argmax(-1)
        self._count(28)
        return 0

    def pdn_sample_rows_f32(self, logits, rs, B, V, params, t, out, stream):
        return self._sample_rows(logits, rs, B, V, params, t, out)

    def pdn_decode_sample_tick_f32(self, logits, rs, B, V, params, ids, pos, hist, emb, emb_rs, D, x_next, stream):
        if B == 0:
            return 0
        p = int(flat(pos, 1, np.int32)[0]) if pos else 0
        self._sample_rows(logits, rs, B, V, params, p, ids)
        tok = np.array(flat(ids, B, np.int64))
        if hist:
            flat(int(flat(hist, 1, np.int64)[0]) + 8 * p * B, B, np.int64)[...] = tok
        if emb:
            for b in range(B):
                flat(x_next, B * D).reshape(B, D)[b] = flat(emb + 4 * int(tok[b]) * emb_rs, D)
        if pos:
            flat(pos, 1, np.int32)[0] += 1
        return 0
