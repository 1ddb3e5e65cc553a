"""CPU: the oracle's detector parameters away from their defaults — the proof that tests/test_gpu_parameters.py can fail.

(1) Mutants of the EWMA recurrence e = (1 - alpha) * e + alpha * x, the ways a kernel can get it subtly wrong: (a) alpha and
1 - alpha swapped, (b) 0.5 hard-coded, (c) a fused multiply-add in place of the two roundings, (d) alpha rounded through float32.
At every alpha the GPU tests pin (except 1.0) each of them leaves the oracle's bits; at the default 0.5 — both products exact,
1 - alpha == alpha — none of them does, which is why a suite that runs the default alone cannot see them.

(2) The oracle's parameters against definitions that are not its own: dbscan_noise_1d(eps, min_samples) against sklearn,
calculate_ewma(alpha) against pandas' ewm and against exact rational arithmetic rounded once per operation."""
from fractions import Fraction

import numpy as np
import pytest

from oracle import tad_oracle as orc

ALPHAS = (0.3, 1 / 3, 0.05, 0.9)          # tests/test_gpu_parameters.py runs these and 1.0
DBSCAN_PARAMS = ((5e5, 4), (2.5e6, 4), (2.5e6, 9), (4e9, 12), (2.0**64, 1), (2.0**64, 4), (2.0**64, 60), (0.5, 2))


def mutant_swapped(x, alpha):
    e, out = 0.0, []
    for v in x:
        e = alpha * e + (1 - alpha) * float(v)
        out.append(e)
    return out


def mutant_hard_coded_half(x, alpha):
    return orc.calculate_ewma(x, 0.5)


def mutant_fma(x, alpha):
    """fma(1 - alpha, e, fl(alpha * x)): the sum of the exact product and the rounded one, rounded once (Fraction -> float is
    correctly rounded; math.fma needs Python 3.13)"""
    e, out = 0.0, []
    for v in x:
        e = float(Fraction(1 - alpha) * Fraction(e) + Fraction(alpha * float(v)))
        out.append(e)
    return out


def mutant_float32_alpha(x, alpha):
    return orc.calculate_ewma(x, float(np.float32(alpha)))


def mutant_incremental(x, alpha):
    e, out = 0.0, []
    for v in x:
        e = e + alpha * (float(v) - e)
        out.append(e)
    return out


MUTANTS = {"swapped": mutant_swapped, "hard_coded_half": mutant_hard_coded_half, "fma": mutant_fma, "float32_alpha": mutant_float32_alpha}


@pytest.fixture(scope="module")
def series():
    """the sum series of the first 50 keys of the table tests/test_gpu_parameters.py runs its jobs on"""
    k, t, v = orc.synth_rows(0, 400_000, 9000, 40)
    pk, pt, pv = orc.stage0(k, t, v, "sum")
    keys, ptr = orc.series_offsets(pk)
    xf = orc.u64_to_f64(pv)
    assert keys.size == 9000 and pk.size == 241_163 and 16 <= np.diff(ptr).min() and np.diff(ptr).max() <= 37
    return [xf[a:b].tolist() for a, b in zip(ptr[:50], ptr[1:51])]


def differing(series, mutant, alpha):
    """per key: at how many points the mutant leaves the oracle's bits"""
    return np.array([sum(a != b for a, b in zip(mutant(x, alpha), orc.calculate_ewma(x, alpha))) for x in series])


@pytest.mark.parametrize("alpha", ALPHAS)
def test_every_mutant_of_the_recurrence_leaves_the_oracles_bits(series, alpha):
    n_pts = sum(len(x) for x in series)
    diff = {name: differing(series, m, alpha) for name, m in MUTANTS.items()}
    print("alpha %.17g, %d points of %d keys: points that differ %s" % (alpha, n_pts, len(series), {k: int(d.sum()) for k, d in diff.items()}))
    for name in ("swapped", "hard_coded_half", "float32_alpha"):
        assert (diff[name] >= 1).all(), (name, int((diff[name] == 0).sum()))
    assert diff["fma"].sum() >= 1


def test_at_the_default_alpha_no_mutant_is_visible(series):
    for name, m in MUTANTS.items():
        assert differing(series, m, 0.5).sum() == 0, name


def test_mutant_counts_on_three_long_series():
    """the first three keys of the 100 x 250 table (734 points, sum): what each mutant changes at alpha 0.3 and at 0.5, verdict flips
    included — printed for the record; asserted: at 0.3 the swapped and the hard-coded recurrence move verdicts, at 0.5 only the
    incremental form e + alpha * (x - e) differs at all"""
    k, t, v = orc.synth_rows(0, 100003, 100, 250)
    pk, pt, pv = orc.stage0(k, t, v, "sum")
    keys, ptr = orc.series_offsets(pk)
    xf = orc.u64_to_f64(pv)
    sigma, _ = orc.stddev_samp_all(xf, ptr)
    xs = [xf[a:b].tolist() for a, b in zip(ptr[:3], ptr[1:4])]
    everything = dict(MUTANTS, incremental=mutant_incremental)
    counts = {}
    for alpha in (0.3, 0.5):
        for name, m in everything.items():
            points = flips = 0
            for x, sd in zip(xs, sigma[:3]):
                got, want = np.array(m(x, alpha)), np.array(orc.calculate_ewma(x, alpha))
                points += int((got != want).sum())
                flips += int(((np.abs(np.array(x) - got) > sd) != (np.abs(np.array(x) - want) > sd)).sum())
            counts[alpha, name] = (points, flips)
        print("alpha %.1f, %d points: (points that differ, verdicts that flip) %s"
              % (alpha, sum(len(x) for x in xs), {n: counts[alpha, n] for n in everything}))
    assert counts[0.3, "swapped"][1] > 0 and counts[0.3, "hard_coded_half"][1] > 0
    assert all(counts[0.3, n][0] > 0 for n in everything)
    assert all(counts[0.5, n] == (0, 0) for n in MUTANTS) and counts[0.5, "incremental"][0] > 0


def seeded_series(trial, rng):
    """1 .. 80 values around 4e9 whose scatter is of the order of one of the eps values, with duplicates and an outlier now and then"""
    n = int(rng.integers(1, 81))
    scale = (2.0, 1e6, 5e6, 6e8, 8e9)[trial % 5]
    x = np.floor(4e9 + rng.uniform(-scale, scale, size=n)) + 8e9
    if trial % 3 == 0:
        x[rng.integers(0, n)] *= 3
    if trial % 4 == 0 and n > 3:
        x[rng.integers(0, n, size=n // 3)] = x[0]
    return x


def test_dbscan_parameters_against_sklearn():
    # algorithm="kd_tree": sklearn's own |x_i - x_j| on the coordinates.  The default picks the brute-force search for series of up to
    # 11 points, whose distances come from |x|^2 - 2 x.y + |y|^2: at values of 1e10 that is off by thousands, eps = 0.5 shows it
    from sklearn.cluster import DBSCAN
    rng = np.random.default_rng(17)
    xs = [seeded_series(trial, rng) for trial in range(60)]
    assert min(x.size for x in xs) <= 3 and max(x.size for x in xs) >= 70
    for eps, ms in DBSCAN_PARAMS:
        noise = 0
        for x in xs:
            want = DBSCAN(min_samples=ms, eps=eps, algorithm="kd_tree").fit_predict(x.reshape(-1, 1)) == -1
            got = orc.dbscan_noise_1d(x, eps, ms)
            assert (got == want).all(), (eps, ms, x.size)
            assert (orc.dbscan_noise_all(x, np.array([0, x.size]), eps, ms) == want).all(), (eps, ms, x.size)
            noise += int(want.sum())
        print("eps %g min_samples %d: %d noise points of %d" % (eps, ms, noise, sum(x.size for x in xs)))


def ewma_rational(x, alpha):
    """every operation of the recurrence in exact rational arithmetic, rounded to double once: IEEE *, -, + without any library float"""
    a = Fraction(alpha)
    om = Fraction(float(1 - a))                      # fl(1 - alpha)
    e, out = Fraction(0), []
    for v in x:
        left, right = Fraction(float(om * e)), Fraction(float(a * Fraction(float(v))))
        e = Fraction(float(left + right))
        out.append(float(e))
    return out


@pytest.mark.parametrize("alpha", ALPHAS + (1.0, 0.5))
def test_ewma_alpha_against_pandas_and_exact_arithmetic(series, alpha):
    for x in series[:20] + [[7.0], [2.0**64, 1.0, 3.0]]:
        want = orc.calculate_ewma(x, alpha)
        assert want == ewma_rational(x, alpha)
        try:
            import pandas as pd
        except ImportError:
            continue
        # pandas turns alpha into a centre of mass and back: the alpha its recurrence runs on is `seen`, an ulp from alpha for 1/3,
        # 0.05 and 0.9, and the bits to expect are the oracle's at that alpha.  pandas starts at y_0 = x_0, the reference at
        # e_{-1} = 0, i.e. e_0 = alpha * x_0
        seen = 1.0 / (1.0 + (1.0 - alpha) / alpha)
        y = pd.Series([seen * x[0]] + list(x[1:]), dtype="float64").ewm(alpha=alpha, adjust=False).mean()
        assert y.tolist() == orc.calculate_ewma(x, seen)
        assert abs(seen - alpha) <= 2.0**-52
