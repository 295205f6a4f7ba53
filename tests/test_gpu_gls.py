"""The periodogram kernels on the device (rvm_gls.hip, rvmcmc/periodogram.py, ChainRecorder.residual_periodogram)
against tests/gls_ref.py.

The power is compared bit for bit (NaN matches NaN) with the restatement run on the device's own rvm_gls_basis
output; the basis' frequencies bit for bit, its sin and cos with 50-digit mpmath at the device's own reduced
phase under 2 x gls_ref.E_TRIG_MEASURED.  Every call runs twice on a workspace filled with 0xFF bytes and must
give the same bits; nothing may be written past an output's last element, between the rows of a padded
power_out, or past the workspace's stated size.

The kernels' size thresholds (rvm_gls.hip), each with a length on either side below:
  GT_SLICE = 16       epochs the product kernel stages through LDS at a time: N = 15 | 16 | 17 (and 33: three
                      slices); an odd N also takes the single-element loads at a row's end;
  GT_F = 64           frequencies of a product block, GP_BLOCK = 64 frequencies of a prepare block: F = 63 | 64 | 65,
                      and 129: three blocks;
  GT_S = 128          series of a product block: S = 127 | 128 | 129; a thread's series pairs are 32 apart and a
                      wave's 16 columns of pairs cover 32 series: S = 63 | 64 | 65 crosses those;
  GC_BLOCK = 256      series of a centre block: S = 255 | 256 | 257;
  GB_BLOCK = 256      threads of a basis block, a pair of epochs each: F ceil(N / 2) = 256 | 258 pairs
                      (test_basis_*); the 16-byte stores need even rows from aligned outputs: odd N and a
                      misaligned output take the 8-byte ones;
  the chunk           gls_chunk_freqs(N) = 64 MiB / (16 bytes x N rounded up to even), rounded down to a multiple
                      of 64: 1048576 frequencies at N = 4 (test_chunks_*).
"""
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before librvmcmc.so is loaded: the process then holds one HIP runtime, torch's)

import gls_ref as G
import summary_ref as R
from conftest import GOLDEN, S2_PLANETS, s2_obs_oracle
from support import rvm_lib, state_scales, to_device, torch_or_fail as _torch

gpu = pytest.mark.gpu

GT_SLICE, GT_F, GT_S, GC_BLOCK, GB_BLOCK = 16, 64, 128, 256, 256
CHUNK_N4 = (64 << 20) // (16 * 4) // 64 * 64


def _dev(a, dtype=np.float64):
    return to_device(a, dtype, copy=True)


def _device_basis(tau, f0, df, k0, F, misalign=False):
    """rvm_gls_basis twice: (cos [F][N], sin [F][N], freq [F]) host arrays."""
    torch = _torch()
    L, lib = rvm_lib()
    N = len(tau)
    td = _dev(tau)
    outs = []
    for _ in range(2):
        off = 1 if misalign else 0
        c = torch.full((off + F * N + 4,), -7.0, dtype=torch.float64, device="cuda")
        s = torch.full((off + F * N + 4,), -7.0, dtype=torch.float64, device="cuda")
        f = torch.full((F + 4,), -7.0, dtype=torch.float64, device="cuda")
        assert c.data_ptr() % 16 == 0 and s.data_ptr() % 16 == 0
        rc = lib.rvm_gls_basis(td.data_ptr(), N, f0, df, k0, F, c.data_ptr() + 8 * off, s.data_ptr() + 8 * off,
                               f.data_ptr(), L.stream_handle())
        assert rc == 0, lib.rvm_last_error()
        torch.cuda.synchronize()
        for t in (c, s):
            assert bool((t[:off] == -7.0).all()) and bool((t[off + F * N:] == -7.0).all())
        assert bool((f[F:] == -7.0).all())
        outs.append([t.cpu().numpy() for t in (c[off:off + F * N].view(F, N), s[off:off + F * N].view(F, N), f[:F])])
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a.view(np.uint64), b.view(np.uint64))
    return outs[0]


def _device_power(tau, w, data, model, S, f0, df, k0, F, float_mean, model_ld=None, power_ld=None, want_freq=True,
                  keep_on_device=False):
    """rvm_gls_power twice on a 0xFF-filled workspace: (power [F][S], freq [F] | None)."""
    torch = _torch()
    L, lib = rvm_lib()
    N = len(tau)
    model_ld = S if model_ld is None else model_ld
    power_ld = S if power_ld is None else power_ld
    td, wd, dd = _dev(tau), _dev(w), _dev(data)
    md = None
    if model is not None:
        m = np.full((N, model_ld), 1e30)  # (a read outside the S columns shows)
        m[:, :S] = model
        md = _dev(m)
    nws = lib.rvm_gls_workspace_bytes(N, F, S)
    assert nws > 0 and nws % 16 == 0
    outs = []
    for _ in range(2):
        p = torch.full((F * power_ld + 4,), -7.0, dtype=torch.float64, device="cuda")
        f = torch.full((F + 4,), -7.0, dtype=torch.float64, device="cuda")
        ws = torch.full((nws + 32,), 0xFF, dtype=torch.uint8, device="cuda")
        rc = lib.rvm_gls_power(td.data_ptr(), wd.data_ptr(), N, dd.data_ptr(), md.data_ptr() if md is not None else 0,
                               model_ld, S, f0, df, k0, F, int(float_mean), p.data_ptr(), power_ld,
                               f.data_ptr() if want_freq else 0, ws.data_ptr(), L.stream_handle())
        assert rc == 0, lib.rvm_last_error()
        torch.cuda.synchronize()
        assert bool((ws[nws:] == 0xFF).all())  # nothing written past the workspace
        rows = p[:F * power_ld].view(F, power_ld)
        assert bool((p[F * power_ld:] == -7.0).all()) and bool((rows[:, S:] == -7.0).all())
        assert bool((f[F:] == -7.0).all()) and (want_freq or bool((f == -7.0).all()))
        outs.append((rows[:, :S].contiguous(), f[:F]))
    assert torch.equal(outs[0][0].view(torch.int64), outs[1][0].view(torch.int64))  # the same bits
    assert torch.equal(outs[0][1].view(torch.int64), outs[1][1].view(torch.int64))
    p, f = outs[0]
    if keep_on_device:
        return p, f
    return p.cpu().numpy(), (f.cpu().numpy() if want_freq else None)


def _assert_same_bits(got, want, msg=""):
    """The same bits, a NaN matching any NaN (IEEE leaves a NaN's sign and payload open)."""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=msg)
    np.testing.assert_array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64), err_msg=msg)


def _case(rng, N, S, scale=1e-4, w_span=4.0):
    """(tau, w, data, model [N][S]): a sinusoid with noise observed at random epochs, and S models that leave
    residuals of a few sigma."""
    t = np.sort(rng.uniform(0.0, 60.0, N))
    tau = t - (t.min() + t.max()) / 2.0
    sigma = 0.05 * scale * np.exp(rng.uniform(0.0, 0.5 * np.log(w_span), N))
    w = G.normalised_weights(sigma)
    data = scale * np.sin(2 * np.pi * t / 9.1 + 0.3) + sigma * rng.standard_normal(N)
    model = data[:, None] - 3.0 * sigma[:, None] * rng.standard_normal((N, S)) \
        - 0.1 * scale * np.cos(2 * np.pi * t[:, None] / (5.0 + np.arange(S)[None, :] % 7))
    return tau, w, data, model


def _assert_power(tau, w, data, model, S, f0, df, k0, F, float_mean, ks=None, **layout):
    """Device power and frequencies against the restatement on the device's own basis, bit for bit, at the rows
    ks (default: all)."""
    got, freq = _device_power(tau, w, data, model, S, f0, df, k0, F, float_mean, **layout)
    # the whole basis in one call, or chosen rows one at a time (they may be far apart)
    blocks = [(0, F)] if ks is None else [(k, 1) for k in ks]
    for k, n in blocks:
        c, s, f = _device_basis(tau, f0, df, k0 + k, n)
        np.testing.assert_array_equal(f, G.phase(tau, f0, df, k0, range(k, k + n))[0])
        np.testing.assert_array_equal(freq[k:k + n], f)
        want = G.power(c, s, w, data, model, float_mean, n_series=S)
        _assert_same_bits(got[k:k + n], want, f"k={k} float_mean={float_mean} k0={k0} {layout}")
    return got


SHAPES = ([(n, 2, 2) for n in (4, 5, GT_SLICE - 1, GT_SLICE, GT_SLICE + 1)] + [(2 * GT_SLICE + 1, 3, 3)]
          + [(4, 1, 1), (4, GT_F - 1, 2), (4, GT_F, 2), (4, GT_F + 1, 2), (5, 2 * GT_F + 1, 1)]
          + [(4, 2, 63), (4, 2, 64), (4, 2, 65), (4, 1, GT_S - 1), (4, 1, GT_S), (4, 1, GT_S + 1), (4, 1, GC_BLOCK - 1),
             (4, 1, GC_BLOCK), (5, 1, GC_BLOCK + 1)])


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d-F%d-S%d" % s)
def test_power_bit_for_bit(shape):
    N, F, S = shape
    tau, w, data, model = _case(np.random.default_rng(N + 100 * F + 10000 * S), N, S)
    f0, df = 0.0131, 0.0037
    # (float_mean, k0, model given, padded): the tight layout, and leading dimensions S + 3 and S + 1 -- odd for
    # even S -- with every mean mode and with and without a model
    combos = [(True, 0, True, False), (True, 0, False, True), (True, 7, True, True), (True, 7, False, False),
              (False, 0, True, True), (False, 0, False, False), (False, 7, True, False), (False, 7, False, True)]
    for float_mean, k0, given, padded in combos:
        layout = dict(model_ld=S + 3, power_ld=S + 1) if padded else {}
        got = _assert_power(tau, w, data, model if given else None, S, f0, df, k0, F, float_mean, **layout)
        assert np.all(np.isfinite(got)) and np.all(got >= -1e-12) and np.all(got <= 1.0 + 1e-12)
        if not given:
            np.testing.assert_array_equal(got, np.repeat(got[:, :1], S, 1))  # S copies of the data's own


@gpu
def test_contents_nan_columns_scales_and_weights():
    rng = np.random.default_rng(5)
    N, F, S = 9, 3, 5
    for scale, w_span in ((1e-4, 4.0), (1.0, 4.0), (1e-4, 1e4), (1.0, 1e4)):
        tau, w, data, model = _case(rng, N, S, scale, w_span)
        if w_span > 100:
            assert w.max() / w.min() > 1e2
        model[3, 1] = np.nan      # one NaN in column 1: the column's powers are NaN, the others' are not
        model[:, 3] = data        # a perfect model: z = 0, YY = 0, 0 / 0
        for float_mean in (True, False):
            got = _assert_power(tau, w, data, model, S, 0.02, 0.011, 0, F, float_mean, model_ld=S + 1, power_ld=S + 2)
            assert np.isnan(got[:, [1, 3]]).all() and np.isfinite(got[:, [0, 2, 4]]).all()


@gpu
def test_chunks_and_split_calls():
    """N = 4, S = 2, F = the chunk + 70: one call equals two calls split at k = 300001, bit for bit, and the rows
    either side of the chunk's edge are the restatement's."""
    torch = _torch()
    N, S, F, split, k0 = 4, 2, CHUNK_N4 + 70, 300001, 7
    tau, w, data, model = _case(np.random.default_rng(44), N, S)
    f0, df = 0.0131, 1e-7
    whole, fw = _device_power(tau, w, data, model, S, f0, df, k0, F, True, keep_on_device=True)
    a, fa = _device_power(tau, w, data, model, S, f0, df, k0, split, True, keep_on_device=True)
    b, fb = _device_power(tau, w, data, model, S, f0, df, k0 + split, F - split, True, keep_on_device=True)
    assert torch.equal(whole.view(torch.int64), torch.cat([a, b]).view(torch.int64))
    assert torch.equal(fw.view(torch.int64), torch.cat([fa, fb]).view(torch.int64))
    edge = [0, split - 1, split, CHUNK_N4 - 2, CHUNK_N4 - 1, CHUNK_N4, CHUNK_N4 + 1, F - 1]
    rows, freq = whole[edge].cpu().numpy(), fw[edge].cpu().numpy()
    for j, k in enumerate(edge):
        c, s, f = _device_basis(tau, f0, df, k0 + k, 1)
        np.testing.assert_array_equal(freq[j:j + 1], f)
        np.testing.assert_array_equal(f, G.phase(tau, f0, df, k0, [k])[0])
        want = G.power(c, s, w, data, model, True)
        _assert_same_bits(rows[j:j + 1], want, f"k={k}")


# ---- the basis ------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("N,F", [(4, 1), (5, 3), (GB_BLOCK - 1, 2), (GB_BLOCK, 2), (GB_BLOCK + 1, 2), (2, GB_BLOCK + 1)])
@pytest.mark.parametrize("k0", [0, 7, 2 ** 53 - 300])
def test_basis_grid_bit_for_bit(N, F, k0):
    """freq_out is the restatement's f_k bit for bit, and the restatement's x and r follow from it; sin and cos at
    that r are mpmath's within the bound.  A wrong x or r would be wrong by far more."""
    assert G.E_TRIG_MEASURED is not None
    rng = np.random.default_rng(N + F)
    tau = rng.uniform(-40.0, 40.0, N)
    f0, df = (0.0131, 0.0037) if k0 < 100 else (0.0131, 2.0 ** -60)
    want_f, _, r = G.phase(tau, f0, df, k0, range(F))
    for misalign in (False, True):
        c, s, f = _device_basis(tau, f0, df, k0, F, misalign)
        np.testing.assert_array_equal(f.view(np.uint64), want_f.view(np.uint64))
        err = G.trig_error_units(s, c, r)
        assert err <= 2 * G.E_TRIG_MEASURED, err


def _trig_arguments():
    """x = tau at f = 1: r spread over [-1/2, 1/2] with 0, +-1/4, +-1/2 and their neighbours, alone and on top of
    whole cycles up to 10^6."""
    rng = np.random.default_rng(9)
    special = []
    for v in (0.0, 0.25, 0.5, 0.125, 0.375):
        for sgn in (1.0, -1.0):
            x = sgn * v
            special += [x, np.nextafter(x, np.inf), np.nextafter(x, -np.inf)]
    special = np.array(special)
    whole = np.array([0.0, 1.0, -1.0, 2.0, 1000.0, -1001.0, 999999.0, -1e6, 1e6])
    lattice = (whole[:, None] + special[None, :]).ravel()
    spread = np.concatenate([rng.uniform(-0.5, 0.5, 1500), rng.uniform(-1e6, 1e6, 1200),
                             rng.uniform(-0.5, 0.5, 300) * 2.0 ** -rng.integers(1, 60, 300)])
    x = np.concatenate([lattice, spread])
    assert len(x) <= 3400
    return x


@gpu
def test_basis_trig_against_mpmath():
    """The device library's sincospi over the sample: the measured figure is printed, then held to
    2 x gls_ref.E_TRIG_MEASURED; and whether the quarter turns are exact, as gls_ref records it."""
    x = _trig_arguments()
    c, s, f = _device_basis(x, 1.0, 0.0, 0, 1)
    assert f[0] == 1.0
    _, xr, r = G.phase(x, 1.0, 0.0, 0, [0])
    np.testing.assert_array_equal(xr[0], x)
    assert np.abs(r).max() == 0.5 and (r == 0.25).any() and (r == -0.25).any() and (r == 0.0).any()
    err = G.trig_error_units(s[0], c[0], r[0])
    q = {0.0: (0.0, 1.0), 0.25: (1.0, 0.0), -0.25: (-1.0, 0.0), 0.5: (0.0, -1.0), -0.5: (0.0, -1.0)}
    exact = all(bool(np.all(s[0][r[0] == rv] == sv) and np.all(c[0][r[0] == rv] == cv)) for rv, (sv, cv) in q.items())
    print(f"sincospi(2 r): max |device - mpmath| = {err:.4f} x 2^-53 over {len(x)} arguments; "
          f"exact at 2 r in {{0, +-1/2, +-1}}: {exact}")
    assert G.E_TRIG_MEASURED is not None
    assert err <= 2 * G.E_TRIG_MEASURED
    assert exact == G.TRIG_EXACT_AT_QUARTERS
    assert np.all(np.abs(s) <= 1.0) and np.all(np.abs(c) <= 1.0)


# ---- refusals: each before any HIP call (they need no device), each naming its argument ----------------------

def test_refusals_name_their_argument():
    from rvmcmc import _lib

    lib = _lib.load()
    P = 0x10000  # a 16-byte aligned address nothing reads
    NAN, INF = float("nan"), float("inf")
    basis = dict(tau=P, n_obs=5, f0=0.1, df=0.01, k0=0, n_freq=3, cos_out=P, sin_out=P, freq_out=P, stream=None)
    power = dict(tau=P, w=P, n_obs=5, data=P, model=P, model_ld=4, n_series=4, f0=0.1, df=0.01, k0=0, n_freq=3,
                 float_mean=1, power_out=P, power_ld=4, freq_out=P, workspace=P, stream=None)
    over = 2 * _lib.RVM_MAX_EPOCHS_PER_DIRECTION + 1
    grid = [(dict(n_freq=0), b"n_freq"), (dict(k0=-1), b"k0"), (dict(k0=2 ** 53 - 2), b"k0 + n_freq"),
            (dict(f0=NAN), b"f0"), (dict(f0=INF), b"f0"), (dict(df=NAN), b"df"), (dict(df=-INF), b"df"),
            (dict(n_obs=0), b"n_obs"), (dict(n_obs=over), b"n_obs"), (dict(tau=None), b"null tau")]
    cases = [("rvm_gls_basis", basis, grid + [(dict(cos_out=None), b"null cos_out"),
                                              (dict(sin_out=None), b"null sin_out")]),
             ("rvm_gls_power", power, grid + [(dict(w=None), b"null w"), (dict(data=None), b"null data"),
                                              (dict(power_out=None), b"null power_out"),
                                              (dict(workspace=None), b"null workspace"),
                                              (dict(workspace=P + 8), b"workspace"),
                                              (dict(n_series=0), b"n_series"), (dict(model_ld=3), b"model_ld"),
                                              (dict(power_ld=3), b"power_ld"), (dict(float_mean=2), b"float_mean"),
                                              (dict(float_mean=-1), b"float_mean")])]
    for name, base, rows in cases:
        fn = getattr(lib, name)
        for change, text in rows:
            rc = fn(*dict(base, **change).values())
            msg = lib.rvm_last_error()
            assert rc < 0 and msg.startswith(name.encode() + b": ") and text in msg, (name, change, rc, msg)
    # k0 + n_freq = 2^53 itself is allowed: the next check answers
    assert lib.rvm_gls_basis(*dict(basis, k0=2 ** 53 - 3, cos_out=None).values()) < 0
    assert b"null cos_out" in lib.rvm_last_error()
    # a null model needs no model_ld; a null freq_out is allowed: the next check answers
    assert lib.rvm_gls_power(*dict(power, model=None, model_ld=0, freq_out=None, workspace=None).values()) < 0
    assert b"null workspace" in lib.rvm_last_error()
    assert lib.rvm_gls_workspace_bytes(0, 3, 4) == 0 and lib.rvm_gls_workspace_bytes(over, 3, 4) == 0
    assert lib.rvm_gls_workspace_bytes(5, 0, 4) == 0 and lib.rvm_gls_workspace_bytes(5, 3, 0) == 0
    assert lib.rvm_gls_workspace_bytes(5, 3, 4) > 0


# ---- the Python layer ---------------------------------------------------------------------------------------

@gpu
def test_gls_of_hd155358():
    """periodogram.gls on the 122 HD155358 velocities: the default grid's 305 frequencies, the peak at planet b,
    and the host restatement (mpmath's basis) within the bound scipy is held to."""
    import oracle as O
    from rvmcmc import periodogram as PG

    obs = O.obs_from_file(os.path.join(GOLDEN, "HD155358.vels"))
    pg = PG.gls(obs)
    assert pg.freq.shape == pg.power.shape == (305,)
    assert abs(pg.period_days[np.argmax(pg.power)] - 193.9) < 0.5
    ks = [0, 1, 40, int(np.argmax(pg.power)), 304]
    t = np.concatenate([obs.tf, obs.tb])
    rv, er = np.concatenate([obs.rvf, obs.rvb]), np.concatenate([obs.errorf, obs.errorb])
    f0, df, F = PG.freq_grid(t)
    tau = t - (t.min() + t.max()) / 2.0
    f, _, r = G.phase(tau, f0, df, 0, ks)
    np.testing.assert_array_equal(pg.freq[ks], f)
    s, c = G.trig_double(r)
    want = G.power(c, s, G.normalised_weights(er), rv, None, True)[:, 0]
    assert np.max(np.abs(pg.power[ks] - want)) <= 1e-12


@gpu
def test_residual_periodogram_end_to_end():
    """The S2 system observed (gls_ref.E2E_*), sampled with planet 1 alone at its true parameters: what is left
    peaks at planet 2."""
    from rvmcmc import _lib, periodogram as PG
    from rvmcmc.chain import ChainRecorder
    from rvmcmc.ensemble import EnsembleSampler
    from rvmcmc.state import State

    obs = s2_obs_oracle(G.E2E_SEED, G.E2E_NPOINTS)
    s = State(planets=[dict(S2_PLANETS[0])])
    rng = np.random.default_rng(3)
    W = 32
    X0 = s.get_params() + 1e-4 * state_scales(s) * rng.standard_normal((W, s.Nvars))
    e = EnsembleSampler(W, s, obs, seed=5)
    e.set_positions(X0)
    rec = ChainRecorder(e, capacity=4)
    e.run_mcmc(4, rec)
    t = np.concatenate([obs.tf, obs.tb])
    rvobs, er = np.concatenate([obs.rvf, obs.rvb]), np.concatenate([obs.errorf, obs.errorb])
    f2 = G.orbital_frequency(S2_PLANETS[1])
    grid = G.grid_around(t, f2)
    S = 16
    pb = rec.residual_periodogram(grid=grid, n_samples=S, return_samples=True)
    F = grid[2]
    assert pb.bands.shape == (5, F) and pb.n_valid.shape == (F,) and pb.data_power.shape == (F,)
    status, rv = pb.status.cpu().numpy(), pb.rv.cpu().numpy()
    assert rv.shape == (len(t), S) and (status == _lib.RVM_STATUS_OK).all()
    np.testing.assert_array_equal(pb.X.cpu().numpy(),
                                  rec.chain().cpu().numpy().transpose(1, 0, 2).reshape(s.Nvars, -1)[:, pb.idx.cpu().numpy()])
    tau, w = PG.series_inputs(t, er)
    c, sn, f = _device_basis(tau, grid[0], grid[1], 0, F)
    np.testing.assert_array_equal(pb.freq, f)
    masked = np.where((status == 0)[None, :], rv, np.nan)
    want_p = G.power(c, sn, w, rvobs, masked, True)
    _assert_same_bits(pb.power.cpu().numpy(), want_p)
    want_b, m = R.rows_quantiles(want_p, pb.q)
    np.testing.assert_array_equal(pb.bands, want_b.T)
    np.testing.assert_array_equal(pb.n_valid, m)
    own = PG.gls(obs, grid=grid)
    np.testing.assert_array_equal(pb.data_power.view(np.uint64), own.power.view(np.uint64))
    np.testing.assert_array_equal(own.power.view(np.uint64), G.power(c, sn, w, rvobs, None, True)[:, 0].view(np.uint64))
    T = float(t.max() - t.min())
    median = pb.bands[list(pb.q).index(0.5)]
    assert abs(pb.freq[np.argmax(median)] - f2) <= 1.0 / T

    # the caller's samples, one with a negative mass: its column is left out of every frequency
    Xs = pb.X.clone()
    Xs[s.get_rawkeys().index("m"), 5] = -1e-3
    pb2 = rec.residual_periodogram(grid=grid, samples=Xs, return_samples=True)
    assert pb2.status.cpu().numpy()[5] == _lib.RVM_STATUS_PRIOR and pb2.idx is None
    assert np.all(pb2.n_valid == S - 1) and np.isnan(pb2.power.cpu().numpy()[:, 5]).all()
    want2, _ = R.rows_quantiles(np.delete(want_p, 5, axis=1), pb2.q)
    np.testing.assert_array_equal(pb2.bands, want2.T)
