"""CPU: the sampled batched decode additions of include/ps_hip.h (ps_hip_sample_rows, ps_hip_model_decode_batch_sampled) are declared in powerserve_amd/hip.py with
the header's argument count, exported by the library, additive to ABI version 2, and reachable through the host facade's driver API."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"ps_hip_sample_rows": 8, "ps_hip_model_decode_batch_sampled": 8}


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
    for name, arity in NEW.items():
        assert want.get(name) == arity, (name, want.get(name))
        assert name in hip.EXPORTS, name
        fn = getattr(L, name)  # exported by the library
        assert fn.argtypes is not None and len(fn.argtypes) == arity, (name, fn.argtypes)
    assert L.ps_hip_abi_version() == 2  # additive: the version and every earlier signature stay


def test_python_wrappers_exist():
    from powerserve_amd import hip, host
    assert callable(getattr(hip.Model, "decode_batch_sampled", None))
    assert callable(getattr(hip, "sample_rows", None))
    assert "psh_model_decode_batch_sampled" in host.EXPORTS and hasattr(host.lib(), "psh_model_decode_batch_sampled")
    assert callable(getattr(host.HostModel, "decode_batch_sampled", None))


def test_facade_checks_column_count_before_the_device():
    """HostModel.decode_batch_sampled refuses mismatched / empty columns before anything reaches the library (no model, no device needed)"""
    from powerserve_amd import host
    hm = host.HostModel.__new__(host.HostModel)  # no model behind it: the check must come first
    with pytest.raises(ValueError):
        hm.decode_batch_sampled([0, 1], [5], 4, [None, None])
    with pytest.raises(ValueError):
        hm.decode_batch_sampled([0, 1], [5, 6], 4, [None])
    with pytest.raises(ValueError):
        hm.decode_batch_sampled([], [], 4, [])
    hm.h = None
