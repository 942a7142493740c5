"""GPU: the two kernels of csrc/trajectory_audit.hip against the numpy restatement the CPU suite pins on the reference's fixture
(tests/trajectory_availability_refs.py).

Cells: every plane compares == (NaN matching NaN) except `within_std`, which must lie within 1 fp32 ulp of the restatement: both compute
it in fp64 and round once, only the order of the fp64 sums differs (the kernel adds hour after hour, numpy pairwise), which moves the
fp64 figure by a few 2^-53 relative, far below half an fp32 ulp but able to flip one rounding.  Medians: == against numpy on the host."""
import numpy as np
import pytest
import torch

from trajectory_availability_refs import cells_ref, golden_cases, median_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
PLANES = ("obs_hours", "total", "recency", "within_std", "endpoint_change")


def _ta():
    from multimodal_edema_prediction_amd import trajectory_availability
    return trajectory_availability


def _medians(planes, take_abs=False):
    from multimodal_edema_prediction_amd.probe_stats import column_medians
    med, valid = column_medians(planes, take_abs)
    return med.cpu().numpy(), valid.cpu().numpy()


def _random_input(seed, N, T, V):
    """Observation probability per variable cycling through {0, 0.04, 0.15, 0.5, 0.9, 1}; counts 1-3; values with offsets up to +-15."""
    rng = np.random.default_rng(seed)
    probs = np.array([(0.5, 1.0, 0.04, 0.9, 0.0, 0.15)[j % 6] for j in range(V)])
    observed = rng.random((N, T, V)) < probs[None, None, :]
    values = rng.standard_normal((N, T, V)) + rng.uniform(-15, 15, size=V)[None, None, :]
    counts = rng.integers(1, 4, size=(N, T, V))
    return np.concatenate([np.where(observed, values, 0.0), np.where(observed, counts, 0)], axis=2).astype(np.float32)


def _host(planes):
    out = {k: getattr(planes, k).cpu().numpy().T for k in PLANES}                  # sample-major, as the restatement
    out["per_sample"], out["var_counts"] = planes.per_sample.cpu().numpy(), planes.var_counts.cpu().numpy()
    return out


def _ulp_distance(a, b):
    """fp32 arrays -> the distance in units of the last place (0 where both are NaN)."""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    d = np.abs(np.where(ia < 0, -(ia & 0x7fffffff), ia) - np.where(ib < 0, -(ib & 0x7fffffff), ib))
    both_nan = np.isnan(a) & np.isnan(b)
    assert (np.isnan(a) == np.isnan(b)).all(), "NaN pattern differs"
    return np.where(both_nan, 0, d)


def _assert_cells(got, want, what):
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, f"{what}: {k} {got[k].shape} {got[k].dtype}"
        if k == "within_std":
            worst = int(_ulp_distance(got[k], want[k]).max())
            print(f"{what}: within_std largest distance {worst} ulp (bound 1)")
            assert worst <= 1, f"{what}: within_std is {worst} ulp off"
        else:
            assert np.array_equal(got[k], want[k], equal_nan=got[k].dtype.kind == "f"), f"{what}: {k}"


def _assert_bitwise(a, b, what):
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), f"{what}: {k} is not bit-identical"


CELL_INPUTS = [(c["x"], c["n_timesteps"]) for c in golden_cases()] + [
    (_random_input(1, 33, 7, 1), 7), (_random_input(2, 35, 5, 130), 5), (_random_input(3, 70, 1, 9), 1)]


@pytest.mark.parametrize("x,n_timesteps", CELL_INPUTS, ids=[f"N{x.shape[0]}_T{x.shape[1]}_V{x.shape[2] // 2}_nt{nt}" for x, nt in CELL_INPUTS])
def test_cells_against_the_restatement(x, n_timesteps):
    got = _host(_ta().trajectory_cells(torch.as_tensor(x, device=DEV), n_timesteps))
    _assert_cells(got, cells_ref(x, n_timesteps), "cells")


def test_cells_never_read_an_unobserved_value_and_take_any_n_timesteps():
    x = golden_cases()[0]["x"].copy()
    v = x.shape[2] // 2
    hidden = x[:, :, v:] <= 0
    x[:, :, :v][hidden] = np.where(np.arange(hidden.sum()) % 2 == 0, np.nan, np.inf).astype(np.float32)
    for n_timesteps in (24, 31, 7):                                                  # 7 < T: recency goes negative, as in the reference
        got = _host(_ta().trajectory_cells(torch.as_tensor(x, device=DEV), n_timesteps))
        _assert_cells(got, cells_ref(golden_cases()[0]["x"], n_timesteps), f"NaN / inf hidden, n_timesteps {n_timesteps}")


def test_cells_chunks_and_launches_are_bit_identical():
    ta = _ta()
    x = torch.as_tensor(golden_cases()[0]["x"], device=DEV)                           # 37 samples: 20 + 17
    V = x.shape[2] // 2
    whole, again = _host(ta.trajectory_cells(x, 24)), _host(ta.trajectory_cells(x, 24))
    _assert_bitwise(whole, again, "two launches")
    planes = ta.CellPlanes(V, 37, DEV)
    for k in PLANES:                                                                  # whatever the buffers held before must not show
        getattr(planes, k).fill_(7)
    planes.per_sample.fill_(7)
    ta.trajectory_cells(x[20:], 24, planes, 20)                                       # out of order as well
    ta.trajectory_cells(x[:20], 24, planes, 0)
    _assert_bitwise(_host(planes), whole, "chunks of 20 + 17")


def test_cells_bad_arguments():
    from multimodal_edema_prediction_amd import abi
    ta = _ta()
    x = torch.zeros((4, 3, 6), device=DEV)
    p = ta.CellPlanes(3, 4, DEV)
    args = lambda **kw: [kw.get("x", abi.ptr(x)), kw.get("n", 4), kw.get("T", 3), kw.get("V", 3), 3, kw.get("n0", 0), kw.get("ld", 4),  # noqa: E731
                         abi.ptr(p.obs_hours), abi.ptr(p.total), abi.ptr(p.recency), abi.ptr(p.within_std), abi.ptr(p.endpoint_change),
                         kw.get("ps", abi.ptr(p.per_sample)), abi.ptr(p.var_counts), abi.stream()]
    L = abi.lib()
    assert L.medp_trajectory_cells(*args()) == 0
    for bad in (dict(x=None), dict(ps=None), dict(n=0), dict(T=0), dict(V=-1), dict(n0=-1), dict(ld=3), dict(n0=1)):
        assert L.medp_trajectory_cells(*args(**bad)) < 0, bad
    with pytest.raises(ValueError):
        ta.trajectory_cells(x, 3, p, 2)                                               # ld = 4 < n0 + n = 6
    with pytest.raises(TypeError):
        ta.trajectory_cells(x.double(), 3)


# ------------------------------------------------------------------------------------------------------------------------------
# medians
# ------------------------------------------------------------------------------------------------------------------------------
def _assert_medians(columns, take_abs=False, ld=None, what=""):
    """columns: list of equally long 1-D arrays of one dtype -> one launch, == against the sort-based rule and numpy."""
    N = len(columns[0])
    buf = np.zeros((len(columns), ld or N), dtype=columns[0].dtype)
    if ld:
        buf[:] = np.nan if buf.dtype.kind == "f" else -7                              # what lies between the columns is not read
    buf[:, :N] = np.stack(columns)
    med, valid = _medians(torch.as_tensor(buf, device=DEV)[:, :N], take_abs)
    for j, col in enumerate(columns):
        want, m = median_ref(col, take_abs)
        print(f"{what} column {j}: median {med[j]!r} of {valid[j]} valid (expected {want!r} of {m})")
        assert valid[j] == m
        assert (np.isnan(want) and np.isnan(med[j])) or med[j] == want, f"{what} column {j}: {med[j]!r} != {want!r}"
        if col.dtype.kind == "f" and m:
            with np.errstate(all="ignore"):
                numpys = float(np.nanmedian(np.abs(col) if take_abs else col))
            assert (np.isnan(numpys) and np.isnan(med[j])) or med[j] == numpys                # -0.0 == 0.0: zeros compare by value


@pytest.mark.parametrize("N", [1, 2, 3, 255, 256, 257])
def test_medians_small_lengths(N):
    rng = np.random.default_rng(N)
    cols = [rng.standard_normal(N).astype(np.float32) for _ in range(3)]
    cols.append(np.full(N, np.nan, dtype=np.float32))                                 # all NaN
    cols.append(np.full(N, -2.5, dtype=np.float32))                                   # all equal
    for keep in (1, N // 2, N - 1):                                                   # different NaN counts
        c = rng.standard_normal(N).astype(np.float32)
        c[rng.permutation(N)[:N - max(keep, 0)]] = np.nan
        cols.append(c)
    cols.append(rng.integers(0, 2 ** 32, size=N, dtype=np.uint64).astype(np.uint32).view(np.float32))   # every key byte, both signs, NaNs
    cols.append(np.where(rng.random(N) < 0.5, -0.0, 0.0).astype(np.float32))
    _assert_medians(cols, what=f"fp32 N={N}")
    _assert_medians(cols, take_abs=True, what=f"|fp32| N={N}")
    _assert_medians(cols, ld=N + 13, what=f"fp32 N={N} ld={N + 13}")
    ints = [rng.integers(-50, 50, size=N).astype(np.int32), rng.integers(-2 ** 31, 2 ** 31, size=N).astype(np.int32),
            np.full(N, -3, dtype=np.int32), rng.integers(0, 3, size=N).astype(np.int32)]
    _assert_medians(ints, what=f"int32 N={N}")
    _assert_medians([c for c in ints if c.min() > -2 ** 31], take_abs=True, ld=N + 5, what=f"|int32| N={N}")


def test_medians_past_every_staged_size():
    """N = 70001: above the 16384-row limit of the kernels that sort in LDS and above the 40960 floats LDS could hold at all."""
    N = 70001
    rng = np.random.default_rng(7)
    few = rng.choice(np.array([-1.5, 0.25, 0.5, 3.0, 40.0], dtype=np.float32), size=N)
    wide = (rng.standard_normal(N) * 100).astype(np.float32)
    holes = wide.copy()
    holes[rng.random(N) < 0.3] = np.nan
    _assert_medians([few, wide, holes, few[::-1].copy()], what="fp32 N=70001")
    _assert_medians([few, wide, holes], take_abs=True, ld=N + 3, what="|fp32| N=70001")
    _assert_medians([rng.integers(0, 5, size=N).astype(np.int32), rng.integers(-10 ** 6, 10 ** 6, size=N).astype(np.int32)], what="int32 N=70001")
    # an even count whose two middle values differ: the pass for the smallest key above the lower median runs
    even = np.concatenate([np.full(35000, 1.0, np.float32), np.full(35000, 2.0, np.float32)])
    rng.shuffle(even)
    med, valid = _medians(torch.as_tensor(even[None], device=DEV))
    assert med[0] == 1.5 and valid[0] == 70000


def test_medians_two_launches_are_bit_identical():
    x = torch.as_tensor(np.random.default_rng(5).standard_normal((4, 5000)).astype(np.float32), device=DEV)
    a, b = _medians(x), _medians(x)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_medians_bad_arguments():
    from multimodal_edema_prediction_amd import abi
    from multimodal_edema_prediction_amd.probe_stats import column_medians
    x = torch.zeros((2, 8), device=DEV)
    med, valid = torch.zeros(2, dtype=torch.float64, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    L = abi.lib()
    call = lambda p=abi.ptr(x), ld=8, c=2, n=8, m=abi.ptr(med), v=abi.ptr(valid): L.medp_column_medians(p, ld, c, n, 0, 0, m, v, abi.stream())  # noqa: E731
    assert call() == 0
    assert call(p=None) < 0 and call(m=None) < 0 and call(v=None) < 0 and call(c=0) < 0 and call(n=0) < 0 and call(ld=7) < 0
    assert call(n=2 ** 30 + 1, ld=2 ** 31) < 0                                        # above MEDP_COLUMN_MEDIAN_MAX_N: refused, not launched
    with pytest.raises(TypeError):
        column_medians(x.double())
    with pytest.raises(ValueError):
        column_medians(x[0])
