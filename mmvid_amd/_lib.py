"""ctypes binding of libmmvid_hip.so, derived from its C header.

include/mmvid_hip.h is the one place the ABI is written down: _cdecl.py reads it at import (a few milliseconds) and every argument
list, return type, struct layout and the ABI version below come from it.  That header's list is pinned (tests/test_cdecl_host.py); a new
entry point is added to include/mmvid_hip_ext.h only, which is read and bound the same way (EXT_HEADER, EXT_SIGNATURES).  Two things
the header does not say are stated here: the Python names of the structs, and which `int` results are values rather than error codes.

The product path has NO fallback: importing works anywhere (so host logic is testable on CPU), but the
first kernel call without the library or without a GPU raises.
"""
import ctypes
import os
from ctypes import c_float, c_int, c_int64, c_uint64, c_void_p

from ._cdecl import EXT_HEADER_PATH, HEADER_PATH, parse

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('MMVID_LIB') or os.path.join(HERE, 'libmmvid_hip.so')  # (MMVID_LIB: another build of the same ABI, for same-box A/Bs)

P = c_void_p
I, I64, F, U64 = c_int, c_int64, c_float, c_uint64

# Python class name -> C typedef
STRUCTS = {'TowerLayer': 'mmvid_tower_layer_t', 'TowerCfg': 'mmvid_tower_cfg_t', 'DecodeToken': 'mmvid_decode_token_t',
           'PostLnLayer': 'mmvid_postln_layer_t', 'PostLnCfg': 'mmvid_postln_cfg_t', 'Conv3dCfg': 'mmvid_conv3d_t',
           'VqganOp': 'mmvid_vqgan_op_t', 'DwKind': 'mmvid_dw_kind_t', 'LnReduce': 'mmvid_ln_reduce_t',
           'PosSegment': 'mmvid_pos_segment_t'}
# `int` results that are a value, not an error code (call() must not be used on them); every other return type is one by itself
INT_VALUED = {'mmvid_abi_version', 'mmvid_device_count', 'mmvid_warp_params_bytes', 'mmvid_tower_decode_persistent_supported'}

with open(HEADER_PATH) as _f:
    HEADER = parse(_f.read(), {c: py for py, c in STRUCTS.items()})
if not (set(STRUCTS.values()) <= set(HEADER.structs) and INT_VALUED <= set(HEADER.functions)):
    raise ImportError(f'the STRUCTS / INT_VALUED tables of {__file__} name something {HEADER_PATH} does not declare')
globals().update({py: HEADER.structs[c] for py, c in STRUCTS.items()})

# name -> argtypes of the entry points that return an error code (call() raises on non-zero) ...
SIGNATURES = {n: args for n, (res, args) in HEADER.functions.items() if res is c_int and n not in INT_VALUED}
# ... and name -> (argtypes, restype) of those that return a value
OTHER = {n: (args, res) for n, (res, args) in HEADER.functions.items() if n not in SIGNATURES}

# include/mmvid_hip_ext.h: the entry points added after the list of mmvid_hip.h was pinned (tests/test_cdecl_host.py counts that header's
# functions and the binding tests hold SIGNATURES | OTHER to it).  Same library, same reader, tables of their own; all return an
# error code, so call() serves them as it serves SIGNATURES.
with open(EXT_HEADER_PATH) as _f:
    EXT_HEADER = parse(_f.read())
if EXT_HEADER.structs or EXT_HEADER.constants or set(EXT_HEADER.functions) & set(HEADER.functions) or any(
        res is not c_int for res, _ in EXT_HEADER.functions.values()):
    raise ImportError(f'{EXT_HEADER_PATH} may declare only new functions that return an error code (structs and constants: {HEADER_PATH})')
EXT_SIGNATURES = {n: args for n, (res, args) in EXT_HEADER.functions.items()}

ABI_VERSION = HEADER.constants['MMVID_ABI_VERSION']  # what mmvid_abi_version() of a matching build returns
_lib = None


class MMVIDError(RuntimeError):
    pass


def load():
    """Load the shared library (no GPU needed for loading).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        # torch's ROCm wheel bundles its own libamdhip64; it must be in the process first so that our library
        # binds to the SAME HIP runtime that owns torch's device pointers and streams (loading ours first gives
        # two runtimes and "no ROCm-capable device" at the first launch).
        import torch  # noqa: F401
        if not os.path.exists(LIB_PATH):
            raise MMVIDError(f'{LIB_PATH} is missing: run `python -m mmvid_amd.build` (hipcc, gfx950). '
                             'There is no CPU/PyTorch fallback for the kernels.')
        lib = ctypes.CDLL(LIB_PATH)
        # the version is checked BEFORE any other symbol is bound: a stale build must say "rebuild", not fail on a missing entry point
        ver = getattr(lib, 'mmvid_abi_version', None)
        have = ver() if ver is not None else None
        if have != ABI_VERSION:
            raise MMVIDError(f'{LIB_PATH} has ABI version {have}, this package needs {ABI_VERSION}: '
                             'rebuild with `python -m mmvid_amd.build --force`')
        missing = []

        def bind(name, args, res):
            fn = getattr(lib, name, None)
            if fn is None:
                missing.append(name)
            else:
                fn.argtypes, fn.restype = args, res

        for name, args in SIGNATURES.items():
            bind(name, args, I)
        for name, (args, res) in OTHER.items():
            bind(name, args, res)
        for name, args in EXT_SIGNATURES.items():
            bind(name, args, I)
        # An older build of the same ABI version given through MMVID_LIB (same-box A/Bs against a parent commit) lacks the entry points
        # added since: it loads, and calling one of them raises.  The package's own library must have them all.
        if missing and not os.environ.get('MMVID_LIB'):
            raise MMVIDError(f'{LIB_PATH} lacks {missing[:4]}: rebuild with `python -m mmvid_amd.build --force`')
        lib._mmvid_missing = frozenset(missing)
        _lib = lib
    return _lib


def call(name, *args):
    lib = load()
    if name in lib._mmvid_missing:
        raise MMVIDError(f'{name} is not in {LIB_PATH} (an older build loaded through MMVID_LIB)')
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise MMVIDError(f'{name} failed (rc={rc}): {lib.mmvid_last_error().decode()}')


# ---- deterministic mode: the library option "deterministic" is the one switch; the Python-side dispatch of ops.py reads it back,
# so mmvid_set_option("deterministic", v) from any caller and MMVID_DETERMINISTIC switch the wrappers too
def is_deterministic():
    """True while the training step takes every fp32 sum in a fixed order.  Asked of the library every
    time (one ctypes call, about a microsecond) rather than cached here, so that a direct mmvid_set_option -- tools/ab_multi.py, a C
    caller in the same process -- switches the wrappers too and the two can never disagree."""
    if 'mmvid_get_option' in load()._mmvid_missing:  # (a build from before the mode existed, through MMVID_LIB)
        return False
    v = c_int(0)
    call('mmvid_get_option', b'deterministic', ctypes.byref(v))
    return v.value != 0


def set_deterministic(flag):
    """Switch the deterministic mode of the library and of the Python wrappers.  Returns the previous value.  A GraphedStep keeps
    the mode it was captured with and refuses to replay under the other one."""
    prev = is_deterministic()
    call('mmvid_set_option', b'deterministic', int(bool(flag)))
    return prev


class deterministic:
    """`with mmvid_amd.deterministic():` (or `deterministic(False)`) -- the mode inside the block, the previous one after it."""

    def __init__(self, flag=True):
        self.flag = bool(flag)

    def __enter__(self):
        self.prev = set_deterministic(self.flag)
        return self

    def __exit__(self, *exc):
        set_deterministic(self.prev)
        return False


FAULT_NAMES = ('embedding id outside its table', 'cross-entropy target outside [0, V)', 'token-table row outside its table', 'reserved')


def device_faults(reset=True):
    """Counts of bad indices the kernels met since the last reset (they read row 0 / class 0 instead of faulting).
    Synchronises the device."""
    arr = (ctypes.c_int64 * 4)()
    call('mmvid_device_faults', arr, int(reset))
    return list(arr)


def check_device_faults():
    """Raise if any kernel met an out-of-range index since the last check (the reference's nn.Embedding / cross_entropy
    would have hit a device-side assert).  Call at a point where a device sync is acceptable: between steps, after a bench."""
    counts = device_faults(reset=True)
    bad = [f'{n} x {FAULT_NAMES[i]}' for i, n in enumerate(counts) if n]
    if bad:
        raise MMVIDError('kernels met out-of-range indices: ' + '; '.join(bad))
