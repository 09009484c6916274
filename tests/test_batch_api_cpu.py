"""CPU: the batched-decode additions of include/ps_hip.h are declared in powerserve_amd/hip.py with the header's argument count, exported by the
library, and reachable through the host facade's driver API."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ps_hip_model_seq_reserve", "ps_hip_model_seq_count", "ps_hip_model_seq_position", "ps_hip_model_seq_select",
       "ps_hip_model_decode_batch", "ps_hip_model_decode_batch_greedy"]


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
    for name in NEW:
        assert name in want, name
        assert name in hip.EXPORTS, name
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == want[name], (name, fn.argtypes, want[name])
    assert want["ps_hip_model_decode_batch"] == 6 and want["ps_hip_model_decode_batch_greedy"] == 6
    assert L.ps_hip_model_seq_position.restype is not None  # size_t, not the default int
    assert L.ps_hip_abi_version() == 2  # additive: the version and every earlier signature stay


def test_python_wrappers_exist():
    from powerserve_amd import hip, host
    for m in ("seq_reserve", "seq_count", "seq_position", "seq_select", "decode_batch", "decode_batch_greedy"):
        assert hasattr(hip.Model, m), m
    HL = host.lib()
    for n in ("psh_model_seq_reserve", "psh_model_seq_select", "psh_model_seq_position", "psh_model_decode_batch"):
        assert n in host.EXPORTS and hasattr(HL, n), n
    for m in ("reserve_sequences", "select_sequence", "sequence_position", "decode_batch"):
        assert hasattr(host.HostModel, m), m


def test_facade_checks_column_count_before_the_device():
    """HostModel.decode_batch refuses mismatched / empty columns before anything reaches the library (no model, no device needed)"""
    import pytest

    from powerserve_amd import host
    hm = host.HostModel.__new__(host.HostModel)  # no model behind it: the check must come first
    with pytest.raises(ValueError):
        hm.decode_batch([0, 1], [5])
    with pytest.raises(ValueError):
        hm.decode_batch([], [])
    hm.h = None
