"""TEST-ONLY host emulation of the pdnhip C ABI.

Lets the whole Python front end (hipnp striding / broadcasting / views / indexing, the tape
engine, nn, optim, data-parallel wrapper) run in the GPU-less container: `hipnp` is pointed
at host memory and every `pdn_*` entry point is answered by a NumPy statement of the same
contract (include/pdn_hip.h).  It is NOT a product path: `pydynet_amd` never imports it, and
on the GPU box the `-m gpu` tests exercise the real library.  Numerics here follow NumPy, so
CPU tests compare against the oracle at fp32 round-off.
"""
from pydynet_amd import _lib
from ._base import _NP, _ints, view, flat  # noqa: F401
from ._runtime import RuntimeMixin
from ._gemm import GemmMixin, counters  # noqa: F401
from ._pointwise import PointwiseMixin
from ._attention import AttentionMixin
from ._decode import DecodeMixin
from ._recurrent_norm import RecurrentNormMixin
from ._conv import ConvMixin
from ._clip import ClipMixin
from ._sampling import SamplingMixin, margin, read_sample_params  # noqa: F401
from ._decode_rows import DecodeRowsMixin, candidates, gemm_np  # noqa: F401
from ._extend import ExtendMixin, append_np, copy_prefix_np, draft_np, extend_np, rotate, settle_np  # noqa: F401
from ._beam import BeamMixin
from ._penalty import PenaltyMixin, apply_np, bits_to_rows, penalty_chunks, read_penalty_params, reset_np  # noqa: F401
from ._logprobs import LogprobsMixin, logprobs_chunks, work_bytes  # noqa: F401

# entries of include/pdn_hip.h that the emulator leaves out: `_lib.provides` answers False and the callers take their
# other path (the split-fp16 lm_head, hipGraph capture and its pool) or never ask on this library (the rest)
NOT_EMULATED = (
    "pdn_linear_rowmax_split_supported", "pdn_linear_rowmax_split_workspace_bytes", "pdn_linear_rowmax_split_parts",
    "pdn_linear_rowmax_split_fwd_f32", "pdn_linear_ce_dx_deferred_split_supported",
    "pdn_linear_ce_dx_deferred_split_workspace_bytes", "pdn_linear_ce_dx_deferred_split_f32",
    "pdn_graph_destroy", "pdn_graph_end_capture", "pdn_graph_launch", "pdn_pool_destroy", "pdn_pool_stats",
    "pdn_adam_multi_tick_f32", "pdn_device_info", "pdn_gemm_prof_collect", "pdn_get_device", "pdn_last_error")


class EmulatedLib(RuntimeMixin, GemmMixin, PointwiseMixin, AttentionMixin, DecodeMixin, RecurrentNormMixin, ConvMixin,
                  ClipMixin, SamplingMixin, DecodeRowsMixin, ExtendMixin, BeamMixin, PenaltyMixin, LogprobsMixin):
    """Every `pdn_*` entry point of include/pdn_hip.h but NOT_EMULATED, one mixin per kernel family."""


def remove(monkeypatch, emu, *names):
    """A library without the entries `names` for the rest of the test: each is deleted from the mixin that defines it, so
    `_lib.provides(name)` answers False."""
    for name in names:
        monkeypatch.delattr(next(c for c in type(emu).__mro__ if name in vars(c)), name)


def install(monkeypatch):
    """Point hipnp at the emulated library (host memory); returns the emulator."""
    from pydynet_amd import hipnp
    emu = EmulatedLib()
    monkeypatch.setattr(_lib, "_LIB", emu)
    monkeypatch.setattr(_lib, "is_built", lambda: True)
    monkeypatch.setattr(hipnp, "_ws", {})
    monkeypatch.setattr(hipnp, "_err", {})
    monkeypatch.setattr(hipnp, "_state", {"device": 0, "stream": 0, "streams": {}})
    # recycled handles of a PREVIOUS emulator instance (pinned read-back slots and their events, the side stream with its
    # fork / join events) mean nothing to this one: a loss read through a stale slot returns whatever that host block
    # held last (seen as a wrong first loss in tests/test_dropin_reference_programs.py after the bench.main() tests)
    from pydynet_amd import _hipnp_host, _hipnp_streams
    monkeypatch.setattr(_hipnp_host.read_later, "_free", {})
    monkeypatch.setattr(_hipnp_streams, "_side", {})
    from pydynet_amd.core import fused
    monkeypatch.setattr(fused.qkv_attention, "_rope_tables", {})
    return emu

