"""CPU: the fork / save / restore additions of include/ps_hip.h are declared in powerserve_amd/hip.py with the header's argument counts and reachable through
the host facade, the facade checks its arguments before the library, and the saved state's header (csrc/ps_kv_state.h, built into libps_host.so as
psh_debug_kv_state_check) accepts a well-formed header and refuses every malformed one."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"ps_hip_model_seq_fork": 5, "ps_hip_model_seq_state_bytes": 2, "ps_hip_model_seq_export": 5, "ps_hip_model_seq_import": 4}


def header_args():
    """{symbol: argument count} of every ps_hip_* declaration of the header"""
    src = open(os.path.join(ROOT, "include", "ps_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(ps_hip_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        args = args.strip()
        out[name] = 0 if args in ("", "void") else args.count(",") + 1
    return out


def test_new_symbols_declared_with_header_arity():
    from powerserve_amd import hip
    L = hip.lib()
    want = header_args()
    for name, n in NEW.items():
        assert want.get(name) == n, (name, want.get(name))
        assert name in hip.EXPORTS, name
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n, (name, fn.argtypes)
    assert L.ps_hip_model_seq_state_bytes.restype is C.c_size_t
    assert L.ps_hip_model_seq_position.restype is C.c_size_t
    assert L.ps_hip_model_seq_fork.argtypes[4] is C.c_size_t and L.ps_hip_model_seq_export.argtypes[2] is C.c_size_t
    assert L.ps_hip_abi_version() == 2  # additive: the version and every earlier signature stay


def test_wrappers_exist():
    from powerserve_amd import hip, host
    for m in ("seq_fork", "seq_state_bytes", "seq_export", "seq_import"):
        assert hasattr(hip.Model, m), m
    HL = host.lib()
    for n in ("psh_model_seq_fork", "psh_model_seq_export", "psh_model_seq_import", "psh_debug_kv_state_check"):
        assert n in host.EXPORTS and hasattr(HL, n), n
    for m in ("fork_sequence", "export_sequence", "import_sequence"):
        assert hasattr(host.HostModel, m), m


def test_facade_checks_destinations_before_the_library():
    """HostModel.fork_sequence refuses an empty destination list and the source among the destinations before anything reaches the library (no model behind it)"""
    from powerserve_amd import host
    hm = host.HostModel.__new__(host.HostModel)  # neither a handle nor a library: the checks must come first
    with pytest.raises(ValueError):
        hm.fork_sequence(0, [])
    with pytest.raises(ValueError):
        hm.fork_sequence(1, [0, 1, 2])
    with pytest.raises(ValueError):
        hm.fork_sequence(2, [2], 5)
    hm.h = None


# ---------------------------------------------------------------- the state header
SHAPE = dict(n_layers=3, kv_dim=128, head_size=64)
N_CTX, N_TOK = 1000, 37


def header(magic=b"PSKV", version=1, n_layers=3, kv_dim=128, head_size=64, n_tokens=N_TOK, contract=0):
    """the documented layout (csrc/ps_kv_state.h), packed here and not by the library"""
    h = struct.pack("<4sIIIIQI32x", magic, version, n_layers, kv_dim, head_size, n_tokens, contract)
    assert len(h) == 64
    return np.frombuffer(h, dtype=np.uint8)


def total(n_tokens=N_TOK, n_layers=3, kv_dim=128):
    return 64 + n_layers * 2 * n_tokens * kv_dim * 4


def check(h, nbytes, n_ctx=N_CTX, contract=0):
    from powerserve_amd import host
    return host.kv_state_check(h, n_ctx=n_ctx, contract=contract, nbytes=nbytes, **SHAPE)


def test_header_accepted_and_written_as_documented():
    from powerserve_amd import host
    rc, n, why = check(header(), total())
    assert (rc, n, why) == (0, N_TOK, "")
    assert np.array_equal(host.kv_state_header(3, 128, 64, N_TOK, 0), header())   # the library's writer produces the documented bytes
    assert np.array_equal(host.kv_state_header(3, 128, 64, 2 ** 33 + 5, 1), header(n_tokens=2 ** 33 + 5, contract=1))
    assert check(header(contract=1), total(), contract=1)[0] == 0
    assert check(header(n_tokens=0), 64) == (0, 0, "")                          # an empty state is a header
    assert check(header(n_tokens=N_CTX), total(N_CTX))[0] == 0                  # a full window


@pytest.mark.parametrize("field,value", [("magic", b"PSKW"), ("magic", b"pskv"), ("version", 2), ("version", 0), ("contract", 1), ("n_layers", 2), ("n_layers", 4),
                                         ("kv_dim", 64), ("kv_dim", 129), ("head_size", 128), ("head_size", 32)])
def test_header_refuses_each_field_changed(field, value):
    h = header(**{field: value})
    shape = dict(n_layers=3, kv_dim=128)
    if field in shape:
        shape[field] = value  # (the length the CHANGED header implies: the field itself must be what is refused)
    for nbytes in (total(), total(**shape)):
        rc, n, why = check(h, nbytes)
        assert rc == 2 and n is None and why, (field, value, nbytes)


def test_header_refuses_lengths_and_windows():
    h = header()
    for nbytes in (total() - 1, total() + 1, 0, 63, 64):
        assert check(h, nbytes)[0] == 2, nbytes
    assert check(h[:63], 63)[0] == 2
    assert check(np.zeros(0, dtype=np.uint8), 0)[0] == 2
    assert check(h, total(), n_ctx=N_TOK)[0] == 0
    assert check(h, total(), n_ctx=N_TOK - 1)[0] == 2                         # n_tokens > n_ctx
    assert check(header(n_tokens=N_CTX + 1), total(N_CTX + 1))[0] == 2
    assert check(header(n_tokens=2 ** 63), total())[0] == 2                   # an absurd length is refused by the window, before any size arithmetic
    assert check(header(contract=1), total(), contract=0)[0] == 2 and check(header(), total(), contract=1)[0] == 2
