"""Host-side argument checks of the FFN activation entry points (csrc/ffn_act.hip): no GPU needed, the checks return before any launch."""
import ctypes as C
import os

import pytest

from gamer_amd import _lib

ROW_FORMS = [f"gamer_{act}_{d}_ld{sfx}" for act in ("swiglu", "silu") for d in ("fwd", "bwd") for sfx in ("", "_bf16")] + \
            ["gamer_swiglu_fwd_ld_tbl", "gamer_swiglu_bwd_ld_tbl", "gamer_relu_tbl_fwd", "gamer_relu_tbl_bwd"]
FLAT_FORMS = [f"gamer_swiglu_{d}{sfx}" for d in ("fwd", "bwd") for sfx in ("", "_bf16")]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from gamer_amd import build
        build.build()
    return _lib.load()


def _args(name, sizes):
    """Arguments by kind: `sizes` fills the int64 / int arguments in order (then 1), every pointer but the trailing stream is a
    dummy, non-null and 64-byte aligned (never dereferenced: the call is refused on the host)."""
    kinds, sizes, out = _lib._SIGNATURES[name], list(sizes), []
    for k, t in enumerate(kinds):
        if t is C.c_void_p:
            out.append(None if k == len(kinds) - 1 else C.c_void_p(64))
        elif t in (C.c_int64, C.c_int):
            out.append(sizes.pop(0) if sizes else 1)
        else:
            out.append(t(0))                                   # p_drop, seed
    return out


def test_every_form_refuses_a_tensor_longer_than_the_32_bit_dropout_counter(lib):
    """T * I / 4 (flat: n / 4) = 2^32 quads is one more than the counter of the mask hash holds: the masks would repeat."""
    assert len(ROW_FORMS + FLAT_FORMS) == 16
    T, I = 1 << 20, 1 << 14
    for name in ROW_FORMS + FLAT_FORMS:
        sizes = (2 * I, T, I) if name in ROW_FORMS else (T * I,)
        rc = getattr(lib, name)(*_args(name, sizes))
        msg = lib.gamer_last_error()
        assert rc != 0 and name.encode() + b":" in msg and b"32-bit dropout counter" in msg, (name, msg)
    # one quad fewer is no counter overflow: the next check (here: a null pointer) is what refuses the call
    for name, sizes in (("gamer_silu_fwd_ld", (I, T - 1, I)), ("gamer_swiglu_fwd", (T * I - 4,))):
        args = _args(name, sizes)
        args[0] = None
        assert getattr(lib, name)(*args) != 0 and b"dropout counter" not in lib.gamer_last_error()
