"""CPU dry-run of the engine's host logic: the C ABI is replaced by a stub that only validates
argument counts/types against include/mmae.h, so the whole Python control flow (buffer shapes,
autograd plumbing, gradient routing) runs here without a GPU.  Numbers are garbage by design."""
import ctypes
import hashlib
import json

import torch

from multimae_amd import _lib, ops


class FakeLib:
    def __getattr__(self, name):
        ret, argtypes = _lib._PROTOS[name]

        def fn(*args):
            assert len(args) == len(argtypes), (name, len(args), len(argtypes))
            for i, (a, t) in enumerate(zip(args, argtypes)):
                if t is ctypes.c_void_p:
                    ok = a is None or isinstance(a, (int, ctypes.c_void_p, ctypes.Array)) or type(a).__name__ == 'CArgObject'
                elif t is ctypes.c_float:
                    ok = isinstance(a, (int, float)) and not isinstance(a, bool)
                else:
                    ok = isinstance(a, int)
                assert ok, (name, i, type(a), t)
            if name == 'mmae_abi_version':
                return 7
            if name == 'mmae_struct_size':
                return ctypes.sizeof((_lib.GemmDesc, _lib.BlockDesc, _lib.StackDesc, _lib.AdapterDesc, _lib.OptDesc, _lib.PatchSrc, _lib.DwGroupDesc, _lib.ColsumJob)[args[0]])
            # slab layouts of the composite entry points: enough room for the views the host code cuts out of them
            if name in ('mmae_stack_act_bytes', 'mmae_stack_out_offset'):
                d = args[0]._obj
                per = d.B * d.N * d.D * 4
                return d.L * per + 256 if name == 'mmae_stack_act_bytes' else args[1] * per
            if name == 'mmae_adapter_act_bytes':
                d = args[0]._obj
                return d.B * d.n_q * d.C * d.ph * d.pw * 4 + 256
            if name in ('mmae_stack_tmp_bytes', 'mmae_adapter_tmp_bytes'):
                return 256
            if name == 'mmae_adapter_pat_offset':
                return 0
            if name == 'mmae_loss_split':
                return 8
            if name == 'mmae_layernorm_bwd_nblk':
                return max(1, min(1024, (args[0] + 3) // 4))
            if name in ('mmae_tokens_assemble_bwd_nblk', 'mmae_decoder_build_bwd_nblk'):
                return min(args[0], 256)
            if name == 'mmae_colsum_ws_elems':
                return 256 * args[1]
            if name == 'mmae_last_error':
                return b'stub'
            return 0
        return fn


def _is_ptr(ctype) -> bool:
    return ctype is ctypes.c_void_p


def _addr(v):
    """address held by a pointer-typed argument or field (None / 0 = NULL)"""
    if isinstance(v, ctypes.c_void_p):
        v = v.value
    return int(v) if v else 0


def _num(v):
    return float('%.9g' % v) if isinstance(v, float) else int(v)


def canon_struct(s: ctypes.Structure):
    """A descriptor as the library sees it, without its addresses: every non-pointer field (floats rounded to 9 digits), NULL / non-NULL
    for every pointer field, and the groups of pointer fields that hold the same address."""
    scal, ptrs = {}, {}

    def walk(obj, prefix):
        for name, ctype in obj._fields_:
            v, key = getattr(obj, name), prefix + name
            if _is_ptr(ctype):
                ptrs[key] = _addr(v)
            elif isinstance(v, ctypes.Array):
                for i, e in enumerate(v):
                    if isinstance(e, ctypes.Structure):
                        walk(e, f'{key}[{i}].')
                    elif _is_ptr(v._type_):
                        ptrs[f'{key}[{i}]'] = _addr(e)
                    else:
                        scal[f'{key}[{i}]'] = _num(e)
            else:
                scal[key] = _num(v)
    walk(s, '')
    by_addr = {}
    for k, a in ptrs.items():
        if a:
            by_addr.setdefault(a, []).append(k)
    return {'struct': type(s).__name__, 'fields': scal, 'set': sorted(k for k, a in ptrs.items() if a),
            'same': sorted(sorted(g) for g in by_addr.values() if len(g) > 1)}


def canon_args(name: str, args):
    """The canonical (address-free) form of one library call's arguments."""
    out = []
    for a, t in zip(args, _lib._PROTOS[name][1]):
        if isinstance(a, ctypes.Array):
            out.append({'array': len(a)})
        elif type(a).__name__ == 'CArgObject':
            out.append(canon_struct(a._obj) if isinstance(a._obj, ctypes.Structure) else 'ref')
        elif _is_ptr(t):
            out.append('ptr' if _addr(a) else 'NULL')
        else:
            out.append(_num(a))
    return out


def digest(canon) -> str:
    return hashlib.sha1(json.dumps(canon, sort_keys=True, separators=(',', ':')).encode()).hexdigest()[:8]


class RecordingLib(FakeLib):
    """FakeLib that also records: `names`, every symbol asked for, in order; `calls`, one (symbol, canon_args) per call, taken at
    call time (descriptors are mutated and reused between calls).  Addresses are never recorded."""

    def __init__(self):
        self.__dict__['names'] = []
        self.__dict__['calls'] = []

    def __getattr__(self, name):
        self.__dict__['names'].append(name)
        fn = super().__getattr__(name)

        def rec(*args):
            self.__dict__['calls'].append((name, canon_args(name, args)))
            return fn(*args)
        return rec


def install():
    _lib._lib = FakeLib()
    ops._require_gpu = lambda t, name='tensor': None
    ops._stream = lambda: 0
    ops._device_ok = lambda t: True
    ops._WS_ELEMS[0] = 1024
    from multimae_amd import functions
    functions.ops._require_gpu = ops._require_gpu
