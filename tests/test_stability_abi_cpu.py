"""rvm_stability_init / rvm_stability_advance refuse bad arguments before any HIP call (no GPU here: a refusal
that reached the runtime would not name its argument), and the Python mirror carries them."""
import ctypes as C

import pytest
from support import header_prototypes

from rvmcmc import _lib

P = 0x1000  # a non-null pointer that is never dereferenced: every call below is refused on the host

INIT = dict(n_planets=2, inclined=0, n=8, params=P, hill_factor=1.0, xv=P, ext=P, status=P, steps=P, stream=0)
ADVANCE = dict(n_planets=2, inclined=0, n=8, params=P, hill_factor=1.0, h=0.3, sample_every=4, n_blocks=2, r_max=0.0,
               xv=P, ext=P, status=P, steps=P, n_alive_out=0, stream=0)
SHARED = [("n_planets", 0, b"n_planets"), ("n_planets", 5, b"n_planets"), ("n_planets", -1, b"n_planets"),
          ("inclined", 2, b"inclined"), ("n", 0, b"n must"), ("n", -3, b"n must"), ("params", 0, b"null params"),
          ("hill_factor", -1.0, b"hill_factor"), ("hill_factor", float("nan"), b"hill_factor"),
          ("xv", 0, b"null xv"), ("ext", 0, b"null ext"), ("status", 0, b"null status"), ("steps", 0, b"null steps")]
ADVANCE_ONLY = [("h", 0.0, b"h must"), ("h", -0.1, b"h must"), ("h", float("inf"), b"h must"),
                ("h", float("nan"), b"h must"), ("sample_every", 0, b"sample_every"), ("sample_every", -2, b"sample_every"),
                ("n_blocks", 0, b"n_blocks"), ("n_blocks", -1, b"n_blocks")]


def _call(name, args):
    lib = _lib.load()
    order = [a for _, a in header_prototypes()[name][1]]
    assert set(order) == set(args), (order, sorted(args))
    return getattr(lib, name)(*[args[a] for a in order]), lib.rvm_last_error()


@pytest.mark.parametrize("arg,value,text", SHARED)
def test_init_refusals(arg, value, text):
    rc, msg = _call("rvm_stability_init", dict(INIT, **{arg: value}))
    assert rc < 0 and msg.startswith(b"rvm_stability_init: ") and text in msg, (rc, msg)


@pytest.mark.parametrize("arg,value,text", SHARED + ADVANCE_ONLY)
def test_advance_refusals(arg, value, text):
    rc, msg = _call("rvm_stability_advance", dict(ADVANCE, **{arg: value}))
    assert rc < 0 and msg.startswith(b"rvm_stability_advance: ") and text in msg, (rc, msg)


def test_mirror_and_constants():
    protos = header_prototypes()
    for name, n_args in (("rvm_stability_init", 10), ("rvm_stability_advance", 15)):
        assert name in protos and name in _lib.SIGNATURES
        assert len(protos[name][1]) == len(_lib.SIGNATURES[name][1]) == n_args
        assert _lib.SIGNATURES[name][0] is C.c_int
    assert _lib.RVM_STATUS_ESCAPE == 6 and _lib.ABI_VERSION >= 14
    assert _lib.load().rvm_abi_version() == _lib.ABI_VERSION
