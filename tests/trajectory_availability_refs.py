"""numpy restatement of the trajectory-availability audit (the reference's analysis/trajectory_availability.py) and the helpers its tests
share.  The per-sample loop is the reference's, with ONE deliberate difference: the within-patient std is computed in fp64 and rounded
once to fp32 (the reference runs numpy's fp32 arithmetic).  Medians are sort-based, with numpy's rule written out: NaNs dropped, a and b
the values at sorted ranks (m - 1) // 2 and m // 2, fp32 columns (float32)(a + b) * 0.5f, integer columns (a + b) / 2.0 in fp64.

tests/test_trajectory_availability_refs_cpu.py pins all of it on tests/golden/trajectory_availability.npz (the reference's own output)."""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trajectory_availability.npz")
PV_COLUMNS = ("variable", "n_samples", "any_observed_rate", "trajectory_2plus_rate", "trajectory_3plus_rate", "median_observed_hours",
              "mean_observed_hours", "median_total_measurements", "median_recency_h_if_observed",
              "median_within_patient_std_if_2plus", "median_abs_endpoint_change_if_2plus")
PS_COLUMNS = ("sample_index", "n_variables_observed", "n_variables_with_trajectory_2plus", "n_variables_with_trajectory_3plus",
              "n_observed_variable_hours")
STD_COLUMN = "median_within_patient_std_if_2plus"
STD_ULPS = 16.0                     # the std column: within 16 * 2^-24 * max|value of that variable| of the reference


def cells_ref(x, n_timesteps):
    """x [N, T, 2V] fp32 -> sample-major arrays [N, V]: obs_hours int32, total / recency / within_std / endpoint_change fp32, and
    per_sample [N, 4] int32, var_counts [V, 4] int64.  Values at unobserved cells are never touched."""
    x = np.asarray(x, dtype=np.float32)
    n, _, v2 = x.shape
    v = v2 // 2
    obs_hours = np.zeros((n, v), dtype=np.int32)
    total = np.zeros((n, v), dtype=np.float32)
    recency = np.full((n, v), np.nan, dtype=np.float32)
    within_std = np.full((n, v), np.nan, dtype=np.float32)
    endpoint_change = np.full((n, v), np.nan, dtype=np.float32)
    for i in range(n):
        values, counts = x[i, :, :v], x[i, :, v:]
        observed = counts > 0
        obs_hours[i] = observed.sum(axis=0)
        run = np.zeros(v, dtype=np.float32)
        for t in range(counts.shape[0]):                      # t order, one fp32 add per hour
            run = run + counts[t]
        total[i] = run
        for j in np.flatnonzero(observed.any(axis=0)):
            idx = np.flatnonzero(observed[:, j])
            recency[i, j] = np.float32(n_timesteps - idx[-1])
            vals = values[idx, j]
            if len(idx) >= 2:
                wide = vals.astype(np.float64)
                within_std[i, j] = np.float32(math.sqrt(float(np.sum((wide - wide.sum() / len(wide)) ** 2)) / len(wide)))
                endpoint_change[i, j] = vals[-1] - vals[0]
    per_sample = np.stack([(obs_hours >= 1).sum(1), (obs_hours >= 2).sum(1), (obs_hours >= 3).sum(1), obs_hours.sum(1)], axis=1)
    var_counts = np.stack([(obs_hours >= 1).sum(0), (obs_hours >= 2).sum(0), (obs_hours >= 3).sum(0), obs_hours.sum(0)], axis=1)
    return {"obs_hours": obs_hours, "total": total, "recency": recency, "within_std": within_std, "endpoint_change": endpoint_change,
            "per_sample": per_sample.astype(np.int32), "var_counts": var_counts.astype(np.int64)}


def median_ref(column, take_abs=False):
    """-> (median as fp64, number of valid entries) of a 1-D fp32 or integer column by the rule in the module docstring."""
    column = np.asarray(column)
    if column.dtype.kind == "f":
        column = column.astype(np.float32)
        column = column[~np.isnan(column)]
    if take_abs:
        column = np.abs(column)
    m = len(column)
    if m == 0:
        return float("nan"), 0
    ordered = np.sort(column, kind="stable")
    a, b = ordered[(m - 1) // 2], ordered[m // 2]
    if column.dtype.kind == "f":
        if m % 2:
            return float(a), m                                # numpy averages ONE element
        with np.errstate(over="ignore", invalid="ignore"):
            return float(np.float32(np.float32(a + b) * np.float32(0.5))), m
    return (float(a) + float(b)) / 2.0, m


def audit_ref(x, variable_names, n_timesteps):
    """The whole audit -> (per_variable, per_sample) column dictionaries in the reference's column and row order."""
    c = cells_ref(x, n_timesteps)
    n, v = c["obs_hours"].shape
    med = lambda a, **kw: np.array([median_ref(a[:, j], **kw)[0] for j in range(v)])  # noqa: E731
    total_med = np.array([float("nan") if np.isnan(c["total"][:, j]).any() else median_ref(c["total"][:, j])[0] for j in range(v)])
    columns = {
        "variable": np.array([str(s) for s in variable_names], dtype=object), "n_samples": np.full(v, n, dtype=np.int64),
        "any_observed_rate": c["var_counts"][:, 0] / n, "trajectory_2plus_rate": c["var_counts"][:, 1] / n,
        "trajectory_3plus_rate": c["var_counts"][:, 2] / n, "median_observed_hours": med(c["obs_hours"]),
        "mean_observed_hours": c["var_counts"][:, 3] / n, "median_total_measurements": total_med,
        "median_recency_h_if_observed": med(c["recency"]), STD_COLUMN: med(c["within_std"]),
        "median_abs_endpoint_change_if_2plus": med(c["endpoint_change"], take_abs=True),
    }
    order = sorted(range(v), key=lambda j: (-columns["trajectory_2plus_rate"][j], -columns["any_observed_rate"][j]))
    per_variable = {k: col[order] for k, col in columns.items()}
    per_sample = {"sample_index": np.arange(n, dtype=np.int64)}
    per_sample.update({name: c["per_sample"][:, i].astype(np.int64) for i, name in enumerate(PS_COLUMNS[1:])})
    return per_variable, per_sample


# ------------------------------------------------------------------------------------------------------------------------------
# the fixture
# ------------------------------------------------------------------------------------------------------------------------------
def golden_cases():
    """-> list of dicts: x, names, n_timesteps, per_variable, per_sample (column dictionaries), csv_pv, csv_ps, stdout."""
    z = np.load(GOLDEN)
    cases = []
    for c in range(int(z["n_cases"])):
        p = f"c{c}_"
        cases.append({"x": z[p + "x"], "names": [str(s) for s in z[p + "names"]], "n_timesteps": int(z[p + "n_timesteps"]),
                      "per_variable": {k: (z[p + "pv_" + k].astype(object) if k == "variable" else z[p + "pv_" + k]) for k in PV_COLUMNS},
                      "per_sample": {k: z[p + "ps_" + k] for k in PS_COLUMNS},
                      "csv_pv": str(z[p + "csv_pv"]), "csv_ps": str(z[p + "csv_ps"]), "stdout": str(z[p + "stdout"])})
    return cases


def std_bounds(case):
    """variable name -> 16 * 2^-24 * max|observed value of that variable|: the fp32 error of the reference's own mean and deviation
    arithmetic over T <= 96 terms, about (log2 T + 2) u max|v|, with a factor of two of margin; the median is 1-Lipschitz in its inputs."""
    x = case["x"]
    v = x.shape[2] // 2
    out = {}
    for j, name in enumerate(case["names"]):
        seen = np.abs(x[:, :, j][x[:, :, v + j] > 0])
        out[name] = STD_ULPS * 2.0 ** -24 * (float(seen.max()) if seen.size else 0.0)
    return out


def same(a, b):
    """== with NaN matching NaN (zeros compare equal whatever their sign)."""
    a, b = float(a), float(b)
    return (math.isnan(a) and math.isnan(b)) or a == b


def assert_tables(got, want, bounds, what):
    """Both tables of one audit against the expected ones: column names, order and dtypes; every entry == (NaN matching NaN) except the
    std column, which stays within `bounds[variable]`."""
    for g, w, names in ((got[0], want[0], PV_COLUMNS), (got[1], want[1], PS_COLUMNS)):
        assert tuple(g) == names, f"{what}: columns {tuple(g)}"
        for k in names:
            gk, wk = np.asarray(g[k]), np.asarray(w[k])
            assert gk.shape == wk.shape, f"{what}: {k} has {gk.shape}, expected {wk.shape}"
            if k == "variable":
                assert [str(s) for s in gk] == [str(s) for s in wk], f"{what}: row order {list(gk)} != {list(wk)}"
                continue
            assert gk.dtype == wk.dtype, f"{what}: {k} is {gk.dtype}, expected {wk.dtype}"
            for r, (a, b) in enumerate(zip(gk.tolist(), wk.tolist())):
                if k == STD_COLUMN:
                    bound = bounds[str(want[0]["variable"][r])]
                    assert (math.isnan(a) and math.isnan(b)) or abs(a - b) <= bound, f"{what}: {k}[{r}] = {a!r}, expected {b!r} +- {bound}"
                else:
                    assert same(a, b), f"{what}: {k}[{r}] = {a!r}, expected {b!r}"


def parse_csv(text):
    """CSV text -> (header, rows of string fields)."""
    import csv
    import io
    rows = list(csv.reader(io.StringIO(text)))
    return rows[0], rows[1:]


def assert_csv(got_text, want_text, bounds, what):
    """Field by field text equality; the std column is parsed and compared within its bound (an empty field is NaN)."""
    (gh, gr), (wh, wr) = parse_csv(got_text), parse_csv(want_text)
    assert gh == wh, f"{what}: header {gh}"
    assert len(gr) == len(wr), f"{what}: {len(gr)} rows, expected {len(wr)}"
    for r, (g, w) in enumerate(zip(gr, wr)):
        for name, a, b in zip(wh, g, w):
            if name == STD_COLUMN:
                assert (a == "") == (b == ""), f"{what}: row {r} {name}: {a!r} against {b!r}"
                if a != "":
                    assert abs(float(a) - float(b)) <= bounds[w[0]], f"{what}: row {r} {name}: {a} against {b}"
            else:
                assert a == b, f"{what}: row {r} {name}: {a!r} against {b!r}"
