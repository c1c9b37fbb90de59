"""ctypes binding of ``libpdnhip.so`` -- the only way the Python front end reaches the GPU.

The prototypes are parsed from ``include/pdn_hip.h`` so the header stays the single source
of truth for the C ABI (a CPU test checks that the shared object exports every declared
symbol).  There is deliberately NO fallback: if the library is missing or fails to load,
:func:`lib` raises, and every HIP-device operation in ``pydynet_amd`` fails loudly.
"""
from __future__ import annotations

import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PDN_LIB") or os.path.join(_HERE, "libpdnhip.so")     # PDN_LIB: another build, for same-box A/B runs
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "pdn_hip.h")
# extension entries (prefix pdnx_): exported by the same library and declared in headers of their own (the reason is in
# include/pdn_optim.h); tests/test_optim_abi_cpu.py holds them to the same header = exports = emulation rule as the core ABI
EXT_HEADER_PATHS = (os.path.join(os.path.dirname(_HERE), "include", "pdn_optim.h"),)
# the masked cross entropy (prefix pdnl_, include/pdn_loss.h): a tuple of its own, because tests/test_optim_abi_cpu.py holds
# EXT_HEADER_PATHS to the pdnx_ entries alone; tests/test_loss_abi_cpu.py holds this one to the same rule
LOSS_HEADER_PATHS = (os.path.join(os.path.dirname(_HERE), "include", "pdn_loss.h"),)
# document-masked attention (prefix pdns_, include/pdn_segattn.h): again a tuple of its own, held to the rule by
# tests/test_segattn_abi_cpu.py
SEG_HEADER_PATHS = (os.path.join(os.path.dirname(_HERE), "include", "pdn_segattn.h"),)
# cross entropy with reduction='none' (prefix pdnr_, include/pdn_rowloss.h): likewise, held to the rule by
# tests/test_rowloss_abi_cpu.py
ROWLOSS_HEADER_PATHS = (os.path.join(os.path.dirname(_HERE), "include", "pdn_rowloss.h"),)
# cross entropy with label_smoothing / z_loss (prefix pdnz_, include/pdn_smoothloss.h): likewise, held to the rule by
# tests/test_smoothloss_abi_cpu.py
SMOOTH_HEADER_PATHS = (os.path.join(os.path.dirname(_HERE), "include", "pdn_smoothloss.h"),)
# per-request logit edits of a decode step (prefix pdne_, include/pdn_logitedit.h): likewise, held to the rule by
# tests/test_logitedit_abi_cpu.py
EDIT_HEADER_PATHS = (os.path.join(os.path.dirname(_HERE), "include", "pdn_logitedit.h"),)
# sampling parameters per row (prefix pdnq_, include/pdn_persample.h): likewise, held to the rule by
# tests/test_persample_abi_cpu.py
PERSAMPLE_HEADER_PATHS = (os.path.join(os.path.dirname(_HERE), "include", "pdn_persample.h"),)
# token-FSM constrained decoding of a decode step (prefix pdnf_, include/pdn_fsm.h): likewise, held to the rule by
# tests/test_fsm_abi_cpu.py
FSM_HEADER_PATHS = (os.path.join(os.path.dirname(_HERE), "include", "pdn_fsm.h"),)
# the RMSNorm backward folded into the layer input gradient (prefix pdng_, include/pdn_normgrad.h): likewise, held to the
# rule by tests/test_normgrad_abi_cpu.py
NORMGRAD_HEADER_PATHS = (os.path.join(os.path.dirname(_HERE), "include", "pdn_normgrad.h"),)
# the block norms' outputs never written: projections without xn, weight gradients from (x, w, rms) (prefix pdnp_,
# include/pdn_normplanes.h): likewise, held to the rule by tests/test_normplanes_abi_cpu.py
NORMPLANES_HEADER_PATHS = (os.path.join(os.path.dirname(_HERE), "include", "pdn_normplanes.h"),)
# multi-token stop sequences of a decode step (prefix pdnh_, include/pdn_stopseq.h): likewise, held to the rule by
# tests/test_stopseq_abi_cpu.py
STOPSEQ_HEADER_PATHS = (os.path.join(os.path.dirname(_HERE), "include", "pdn_stopseq.h"),)
# all weight plane images of a training pass in one launch (prefix pdnw_, include/pdn_wimages.h): likewise, held to the
# rule by tests/test_wimages_abi_cpu.py
WIMAGES_HEADER_PATHS = (os.path.join(os.path.dirname(_HERE), "include", "pdn_wimages.h"),)

_CTYPE = {
    "int": ctypes.c_int,
    "int64_t": ctypes.c_int64,
    "float": ctypes.c_float,
    "double": ctypes.c_double,
}


def parse_header(path: str = HEADER_PATH):
    """Return {name: (restype, [argtypes])} for every function declared in the header."""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    protos = {}
    for m in re.finditer(r"(const\s+char\s*\*|int64_t|int)\s+(pdn[xlsrzeqfgphw]?_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.S):
        ret, name, args = m.group(1), m.group(2), m.group(3)
        restype = ctypes.c_char_p if "char" in ret else _CTYPE[ret]
        argtypes = []
        args = args.strip()
        if args and args != "void":
            for a in args.split(","):
                a = a.strip()
                if "*" in a:
                    argtypes.append(ctypes.c_void_p)
                else:
                    base = a.replace("const", "").split()[0]
                    argtypes.append(_CTYPE[base])
        protos[name] = (restype, argtypes)
    return protos


class HipLibraryError(RuntimeError):
    """A `pdn_*` entry point returned non-zero; `code` is that status (negative PDN_E*, positive hipError_t)."""

    def __init__(self, message, code=None):
        super().__init__(message)
        self.code = code


class _Lib:
    def __init__(self):
        if not os.path.exists(LIB_PATH):
            raise HipLibraryError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C pydynet_amd/csrc`). The HIP backend has no CPU fallback.")
        # The library owns its device runtime (allocator, copies, streams, RCCL): nothing but the
        # ROCm HIP runtime it is linked against is needed.  RTLD_GLOBAL so that a HIP runtime loaded
        # later by another package in the same process resolves to the same libamdhip64.
        self.cdll = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        self.protos = parse_header()
        for path in (EXT_HEADER_PATHS + LOSS_HEADER_PATHS + SEG_HEADER_PATHS + ROWLOSS_HEADER_PATHS + SMOOTH_HEADER_PATHS
                     + EDIT_HEADER_PATHS + PERSAMPLE_HEADER_PATHS + FSM_HEADER_PATHS + NORMGRAD_HEADER_PATHS
                     + NORMPLANES_HEADER_PATHS + STOPSEQ_HEADER_PATHS + WIMAGES_HEADER_PATHS):
            self.protos.update(parse_header(path))
        self.fn = {}
        for name, (restype, argtypes) in self.protos.items():
            f = getattr(self.cdll, name)  # AttributeError if the .so lacks a declared symbol
            f.restype = restype
            f.argtypes = argtypes
            self.fn[name] = f
        self._last_error = self.fn["pdn_last_error"]
        self.free = self.fn["pdn_free"]              # hot: called from _Buffer.__del__

    def call(self, name, *args):
        rc = self.fn[name](*args)
        if rc != 0:
            msg = self._last_error()
            raise HipLibraryError(f"{name} failed (code {rc}): {msg.decode() if msg else ''}", rc)

    def query(self, name, *args):
        """For functions that return a value (workspace sizes, counts) rather than a status."""
        return self.fn[name](*args)


_LIB = None


def lib() -> _Lib:
    global _LIB
    if _LIB is None:
        _LIB = _Lib()
    return _LIB


def provides(name: str) -> bool:
    """Whether the installed library answers entry point `name` (an ABI stand-in may implement only part of the header)."""
    L = lib()
    fn = getattr(L, "fn", None)
    return name in fn if fn is not None else hasattr(L, name)


def is_built() -> bool:
    return os.path.exists(LIB_PATH)
