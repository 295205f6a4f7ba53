"""The stretch-move device kernels straight through the C ABI on synthetic inputs, against
tests/stretch_ref.py (bit restatement of z, j, q; accept decisions by the 50-digit margin D) and
tests/philox_ref.py.

No plan, no likelihood launch, no sampler: rvm_stretch_propose / _accept, rvm_pt_stretch_propose / _accept
and rvm_stretch_iteration_end get torch tensors.  Every column of every input differs, so a wrong
[p n + j] index cannot hide; c0, c1, x0_aos and x1_aos are four separate buffers (a rank's window of the
half is passed, where the mirrors cannot alias the complements without the launch racing against itself).

Positions, z, log-probabilities, counters and statuses are compared bit for bit.  A decision is the
reference's wherever |D| > B (stretch_ref's rounding bound, derived there, not tuned on the kernel); the
cases are built so that every walker is (tests/test_stretch_ref_cpu.py asserts it), bracketed ones 64 B from
their threshold.  Each comparison that leans on the margin prints its smallest |D| / B ("RATIO ..." lines,
pytest -s).
"""
import numpy as np
import pytest

import philox_ref
import pt_ref
import stretch_ref as R
from support import rvm_lib as _lib, to_device as _dev, torch_or_fail as _torch

pytestmark = pytest.mark.gpu

SEED = R.SEED
eq = np.testing.assert_array_equal


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _host(*ts):
    _torch().cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in ts]


def _ratio(tag, ratio):
    finite = ratio[np.isfinite(ratio)]
    if finite.size:
        print(f"\nRATIO {tag} min |D|/B = {finite.min():.4g} over {finite.size} walkers", flush=True)
        assert (finite > 1.0).all(), (tag, finite.min())


# ---- a, b. the proposals ------------------------------------------------------------------------


def _propose(P, n0, begin, x, n1, c, a, seed=0, it=0, half=0, draws=None):
    """rvm_stretch_propose on host arrays x [P][n0], c [P][n1]; draws (u1, u2) or None: device Philox."""
    torch = _torch()
    _lib_, lib = _lib()
    xd, cd = _dev(x), _dev(c)
    dd = None if draws is None else _dev(np.concatenate(draws))
    q = torch.full((P, n0), float("nan"), dtype=torch.float64, device="cuda")
    z = torch.full((n0,), float("nan"), dtype=torch.float64, device="cuda")
    _lib_.check(lib.rvm_stretch_propose(P, n0, begin, xd.data_ptr(), n1, cd.data_ptr(), float(a), seed, it, half,
                                        _ptr(dd), q.data_ptr(), z.data_ptr(), _lib_.stream_handle()), "propose")
    return _host(q, z)


def _pt_propose(P, T, Wh, x, c, a, seed=0, it=0, half=0, draws=None):
    torch = _torch()
    _lib_, lib = _lib()
    xd, cd = _dev(x), _dev(c)
    dd = None if draws is None else _dev(np.concatenate(draws))
    q = torch.full((P, T * Wh), float("nan"), dtype=torch.float64, device="cuda")
    z = torch.full((T * Wh,), float("nan"), dtype=torch.float64, device="cuda")
    _lib_.check(lib.rvm_pt_stretch_propose(P, T, Wh, xd.data_ptr(), cd.data_ptr(), float(a), seed, it, half, _ptr(dd),
                                           q.data_ptr(), z.data_ptr(), _lib_.stream_handle()), "pt propose")
    return _host(q, z)


@pytest.mark.parametrize("a", R.PROPOSE_A)
@pytest.mark.parametrize("shape", R.PROPOSE_SHAPES)
@pytest.mark.parametrize("P", R.PROPOSE_P)
def test_propose_injected_draws(P, shape, a):
    """u2 pinned to 2^-54, 1 - 2^-53 and exactly 1.0 (partners 0, n1 - 1 and, by the clamp, n1 - 1), u1 to
    2^-54 and 1.0 (z at 1/a and a); q and z to the bit."""
    n0, n1 = shape
    c = R.propose_case(P, n0, n1, a)
    for u1, u2 in c["draws"]:
        q_ref, z_ref, j = R.propose(c["x"], c["c"], u1, u2, a)
        assert ((j >= 0) & (j < n1)).all()
        eq(j[u2 == 1.0], n1 - 1)
        eq(z_ref[u1 == 1.0], a)
        q, z = _propose(P, n0, 0, c["x"], n1, c["c"], a, draws=(u1, u2))
        eq(z, z_ref)
        eq(q, q_ref)


@pytest.mark.parametrize("shape", R.PT_SHAPES)
@pytest.mark.parametrize("P,a", [(1, 2.0), (10, 2.0), (17, 1.5)])
def test_pt_propose_injected_draws(P, a, shape):
    """u2 = 1.0 at a walker of every temperature: without the clamp its partner would be walker 0 of the next
    temperature (past the array at the last).  Temperatures' columns come from disjoint ranges, and each q
    lies next to its own."""
    T, Wh = shape
    c = R.pt_propose_case(P, T, Wh)
    q_ref, z_ref, cj = R.pt_propose(c["x"], c["c"], c["u1"], c["u2"], a, T, Wh)
    eq(cj // Wh, np.repeat(np.arange(T), Wh))
    q, z = _pt_propose(P, T, Wh, c["x"], c["c"], a, draws=(c["u1"], c["u2"]))
    eq(z, z_ref)
    eq(q, q_ref)
    assert ((q > c["base"] - a) & (q < c["base"] + 1.0 + a)).all()
    if T == 1:  # one temperature: the plain kernel's bits
        q1, z1 = _propose(P, Wh, 0, c["x"], Wh, c["c"], a, draws=(c["u1"], c["u2"]))
        eq(q, q1)
        eq(z, z1)


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("it", [5, 2 ** 32 + 3, 2 ** 47 + 1])
@pytest.mark.parametrize("begin", [0, 1000, R.BIG])
def test_propose_device_philox(begin, it, half):
    """The device's own draws: items and iterations at and above 2^32 use the second and fourth counter
    words."""
    P, n0, n1, a = 3, 70, 33, 2.0
    c = R.propose_case(P, n0, n1, a)
    u1, u2, _ = philox_ref.stretch_uniforms(SEED, begin, n0, it, half)
    q_ref, z_ref, _ = R.propose(c["x"], c["c"], u1, u2, a)
    q, z = _propose(P, n0, begin, c["x"], n1, c["c"], a, SEED, it, half)
    eq(z, z_ref)
    eq(q, q_ref)


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("it", [5, 2 ** 32 + 3, 2 ** 47 + 1])
def test_pt_propose_device_philox(it, half):
    """T = 3: the items t W + h Wh + k."""
    P, T, Wh, a = 3, 3, 11, 2.0
    c = R.pt_propose_case(P, T, Wh)
    items = pt_ref.items(T, 2 * Wh, half).reshape(-1)
    u1, u2 = philox_ref.uniform2_vec(SEED, items, it, philox_ref.RNG_STRETCH_PROPOSE | (half << 8))
    q_ref, z_ref, _ = R.pt_propose(c["x"], c["c"], u1, u2, a, T, Wh)
    q, z = _pt_propose(P, T, Wh, c["x"], c["c"], a, SEED, it, half)
    eq(z, z_ref)
    eq(q, q_ref)


# ---- c, d, e. the accepts -----------------------------------------------------------------------


def _accept(c, T=None, betas=None, counter=True, philox=None):
    """One accept launch of a stretch_ref case: the plain entry (T None) or the tempered one (T temperatures
    of n / T walkers).  philox: (begin, iteration, half) takes u3 from the device."""
    _lib_, lib = _lib()
    P, n = c["P"], c["n"]
    x, lnp = _dev(c["x"]), _dev(c["lnp"])
    q, ln, z = _dev(c["q"]), _dev(c["lnp_new"]), _dev(c["z"])
    u3 = None if philox else _dev(c["u3"])
    acc = _dev(c["accepted"], np.int32) if counter else None
    begin, it, half = philox or (0, 0, 0)
    if T is None:
        _lib_.check(lib.rvm_stretch_accept(P, n, begin, x.data_ptr(), lnp.data_ptr(), q.data_ptr(), ln.data_ptr(),
                                           z.data_ptr(), SEED, it, half, _ptr(u3), _ptr(acc), _lib_.stream_handle()),
                    "accept")
    else:
        b = _dev(np.asarray(betas, dtype=np.float64))
        _lib_.check(lib.rvm_pt_stretch_accept(P, T, n // T, b.data_ptr(), x.data_ptr(), lnp.data_ptr(), q.data_ptr(),
                                              ln.data_ptr(), z.data_ptr(), SEED, it, half, _ptr(u3), _ptr(acc),
                                              _lib_.stream_handle()), "pt accept")
    return _host(x, lnp, acc)


def _check_accept(tag, got, c):
    """x, lnp and the counter against the reference, to the bit: accepted walkers hold q and lnp_new, rejected
    ones what they held (their q is NaN, so a stray copy shows)."""
    x, lnp, acc = got
    ref = c["ref"]
    _ratio(tag, ref["ratio"])
    eq(lnp, ref["lnp"])
    eq(x, ref["x"])
    if acc is not None:
        eq(acc, ref["accepted"])
        eq(acc - c["accepted"], ref["acc"].astype(np.int32))


@pytest.mark.parametrize("kind", ["random", "bracket"])
@pytest.mark.parametrize("n0", R.ACCEPT_N)
@pytest.mark.parametrize("P", R.ACCEPT_P)
def test_accept_injected_u3(P, n0, kind):
    """Random and bracketed log-probabilities (magnitudes 1e-3 .. 1e6) through rvm_stretch_accept, then through
    the tempered entry at one temperature with beta = 1: the same bits."""
    c = R.accept_case(P, n0, kind)
    if n0 > 1:
        assert c["ref"]["acc"].any() and not c["ref"]["acc"].all()
    got = _accept(c)
    _check_accept(f"c {kind} P={P} n0={n0}", got, c)
    pt = _accept(c, T=1, betas=[1.0])
    for g, p in zip(got, pt):
        eq(p, g)


def test_accept_without_a_counter():
    c = R.accept_case(10, 257, "bracket")
    _check_accept("c no counter", _accept(c, counter=False), c)
    _check_accept("c pt no counter", _accept(c, T=1, betas=[1.0], counter=False), c)


@pytest.mark.parametrize("kind", ["random", "bracket"])
@pytest.mark.parametrize("shape", R.PT_ACCEPT_SHAPES)
@pytest.mark.parametrize("P", R.ACCEPT_P)
def test_pt_accept_injected_u3(P, shape, kind):
    """beta = 1, 0.25 and 1e-3 by temperature."""
    T, Wh = shape
    c = R.accept_case(P, Wh, kind, T, R.PT_BETAS)
    assert c["ref"]["acc"].any() and not c["ref"]["acc"].all()
    _check_accept(f"c pt {kind} P={P} T={T} Wh={Wh}", _accept(c, T=T, betas=R.PT_BETAS), c)


@pytest.mark.parametrize("tempered", [False, True])
def test_accept_nonfinite_table(tempered):
    """-inf and NaN proposals reject; a walker at -inf takes a finite proposal (emcee's semantics) and rejects
    a -inf one (D is NaN); u3 = 1.0 (ln u3 = 0) goes by the sign of D alone.  Exact, no margin; the
    neighbours keep their bracketed decisions.  The tempered kernel's lnp_old is finite (include/rvmcmc.h)."""
    c = R.nonfinite_case(tempered)
    eq(c["ref"]["acc"], c["want"])
    got = _accept(c, T=1, betas=[c["beta"][0]]) if tempered else _accept(c)
    _check_accept(f"d tempered={tempered}", got, c)
    eq(got[2], c["want"].astype(np.int32))


@pytest.mark.parametrize("half", [0, 1])
def test_accept_device_philox(half):
    """lnp_new bracketed around the device's own u3 (stream RNG_STRETCH_ACCEPT | half << 8), items from
    2^32 + 7: another stream or a dropped counter word moves the thresholds by far more than the brackets."""
    c = R.accept_case(10, 70, "bracket", 1, None, half, R.BIG, 5)
    _check_accept(f"e half={half}", _accept(c, philox=(R.BIG, 5, half)), c)
    c = R.accept_case(10, 23, "bracket", 3, R.PT_BETAS, half, 0, 5)
    _check_accept(f"e pt half={half}", _accept(c, T=3, betas=R.PT_BETAS, philox=(0, 5, half)), c)


# ---- f. rvm_stretch_iteration_end ----------------------------------------------------------------

OUTS = ("x1", "lnp1", "accepted1", "lnp_new_out", "status_new_out", "x1_aos", "x0_aos")


def _iteration_end(c, nullable=True):
    """One launch on a stretch_ref.iteration_end_case; nullable=False passes NULL for x0_aos, x1_aos,
    accepted1, lnp_new_out and status_new_out."""
    torch = _torch()
    _lib_, lib = _lib()
    n, s0 = c["n"], c["s0_begin"]
    x0, x1, lnp1 = _dev(c["x0"]), _dev(c["x1"]), _dev(c["lnp1"])
    c0, c1 = _dev(c["c0"]), _dev(c["c1"])
    dec_all, dec_pad = _dev(c["dec_all"], np.int32), _dev(c["dec_pad"], np.int32)
    dec_local = dec_pad[s0:s0 + n]  # a window of a whole half's worth of decisions that are not dec_all's
    spec, st = _dev(c["lnp_spec"]), _dev(c["st_spec"], np.int32)
    x0a = _dev(c["x0_aos"]) if nullable else None
    x1a = _dev(c["x1_aos"]) if nullable else None
    acc = _dev(c["accepted1"], np.int32) if nullable else None
    lnew = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda") if nullable else None
    stnew = torch.full((n,), -1, dtype=torch.int32, device="cuda") if nullable else None
    _lib_.check(lib.rvm_stretch_iteration_end(
        c["dim"], n, s0, c["s1_begin"], x0.data_ptr(), _ptr(x0a), dec_local.data_ptr(), dec_all.data_ptr(),
        x1.data_ptr(), _ptr(x1a), lnp1.data_ptr(), c["n_half"], c0.data_ptr(), c1.data_ptr(), spec.data_ptr(),
        st.data_ptr(), float(c["a"]), c["seed"], c["iteration"], _ptr(acc), _ptr(lnew), _ptr(stnew),
        _lib_.stream_handle()), "iteration_end")
    out = dict(zip(OUTS, _host(x1, lnp1, acc, lnew, stnew, x1a, x0a)))
    eq(_host(x0)[0], c["x0"])  # read only
    return out


@pytest.mark.parametrize("shape", R.ITER_END_SHAPES)
@pytest.mark.parametrize("dim", R.ITER_END_DIMS)
def test_iteration_end_matches_reference(dim, shape):
    """Both instantiations (dim <= 16, dim > 16), each with local and remote partners that accepted or
    rejected and with partners on both sides of both edges of the window (the seed and iteration of
    stretch_ref.find_case).  The two variants' log-probabilities sit on opposite sides of the threshold, so the
    wrong variant, the wrong decision array or the wrong draw flips the outcome."""
    c = R.iteration_end_case(dim, *shape)
    ref = c["ref"]
    _ratio(f"f dim={dim} shape={shape}", ref["ratio"])
    got = _iteration_end(c)
    for k in ("lnp_new_out", "status_new_out", "lnp1", "accepted1", "x1", "x1_aos", "x0_aos"):
        eq(got[k], ref[k], err_msg=k)
    n = shape[0]
    eq((got["x1_aos"] == -7777.0).all(axis=1), ~ref["acc"])      # accepted rows written, the others untouched
    eq((got["x0_aos"] == -7777.0).all(axis=1), c["dec_local"] == 0)  # refreshed rows only
    if n > 1:
        assert ref["acc"].any() and not ref["acc"].all()


@pytest.mark.parametrize("dim", [10, 17])
def test_iteration_end_without_the_nullable_outputs(dim):
    c = R.iteration_end_case(dim, 64, 192, 64)
    got = _iteration_end(c, nullable=False)
    eq(got["x1"], c["ref"]["x1"])
    eq(got["lnp1"], c["ref"]["lnp1"])


@pytest.mark.parametrize("shape", [(64, 192, 64), (5, 12, 5), (300, 900, 0)])
@pytest.mark.parametrize("dim", [10, 17])
def test_rebuilt_partner_is_the_proposal_of_walker_j(dim, shape):
    """'The same bits either way': a partner outside the window that accepted is rebuilt from c0, c1 and its
    own draws as exactly the q that rvm_stretch_propose gives walker j of half 0 with the same seed."""
    c = R.iteration_end_case(dim, *shape)
    ref, n_half = c["ref"], c["n_half"]
    q_all, _ = _propose(dim, n_half, 0, np.ascontiguousarray(c["c0"].T), n_half, np.ascontiguousarray(c["c1"].T),
                        c["a"], c["seed"], c["iteration"], 0)
    rebuilt = ~ref["local"] & ref["v"]
    assert rebuilt.any()
    eq(ref["rebuilt"][:, rebuilt], q_all[:, ref["j"][rebuilt]])
    sel = rebuilt & ref["acc"]
    if shape[0] > 5:
        assert sel.sum() >= 2
    got = _iteration_end(c)
    eq(got["x1"][:, sel], R.stretch_q(q_all[:, ref["j"][sel]], ref["z"][sel][None], c["x1"][:, sel]))
