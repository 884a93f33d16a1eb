"""The reduction over a candidate's particle totals, restated in numpy float32 from its definition (include/hipets.h,
hipets_set_particle_reduce) -- one ``np.float32`` operation per line, in the stated order, written from the definitions and not from
the kernel.  ``t`` holds one candidate's P totals in particle order.  The yardstick of tests/test_particle_reduce_host.py and
tests/test_gpu_particle_reduce.py: comparisons are bit for bit, NaN equal to NaN."""
import numpy as np

F = np.float32
KINDS = ("mean", "mean_std", "min", "max", "worst_k")


def _mean(t):
    s = F(0.0)
    for x in t:
        s = F(s + x)
    return F(s / F(len(t)))


def _mean_std(t, kappa):
    m = _mean(t)
    q = F(0.0)
    for x in t:
        d = F(x - m)
        dd = F(d * d)
        q = F(q + dd)
    var = F(q / F(len(t)))
    sd = F(np.sqrt(var))  # (numpy's float32 sqrt is correctly rounded)
    ks = F(F(kappa) * sd)
    return F(m - ks)


def _extreme(t, lowest):
    v = t[0]
    for x in t[1:]:
        better = (x < v) if lowest else (x > v)
        v = x if (better or x != x) else v
    return F(v)


def _worst_k(t, k):
    P = len(t)
    assert 1 <= k <= P
    if any(x != x for x in t):
        return F("nan")
    a = np.array(t, dtype=np.float32)
    s = F(0.0)
    for p in range(P):
        rank = int(np.count_nonzero(a[:p] <= a[p])) + int(np.count_nonzero(a[p + 1:] < a[p]))  # (comparisons only: no rounding)
        if rank < k:
            s = F(s + t[p])
    return F(s / F(k))


def particle_value(t, kind, kappa=0.0, k=0):
    """The value of one candidate: ``t`` float32 [P]."""
    t = [F(x) for x in np.asarray(t, dtype=np.float32).reshape(-1)]
    with np.errstate(all="ignore"):  # inf - inf, inf * 0, overflow: the IEEE results are the expected values
        if kind == "mean":
            return _mean(t)
        if kind == "mean_std":
            return _mean_std(t, kappa)
        if kind in ("min", "max"):
            return _extreme(t, kind == "min")
        if kind == "worst_k":
            return _worst_k(t, int(k))
    raise ValueError(kind)


def particle_reduce(totals, pop, P, kind, kappa=0.0, k=0):
    """totals float32 [pop * P] (row c * P + p) -> float32 [pop]."""
    tot = np.asarray(totals, dtype=np.float32).reshape(pop, P)
    return np.array([particle_value(tot[c], kind, kappa, k) for c in range(pop)], dtype=np.float32)


def same_bits(a, b):
    """Bit for bit, every NaN equal to every NaN."""
    a, b = np.asarray(a, dtype=np.float32).reshape(-1), np.asarray(b, dtype=np.float32).reshape(-1)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32)))


def edge_totals(pop, P, first=0):
    """The totals of the rule's tests for (pop, P): candidate c is case (c + first) % 6 of: normals scaled by 100, integer ties in
    0..3, all totals equal, one NaN particle, one +inf, one -inf (pop < 6: ``first`` = 0..5 brings every case to every candidate)."""
    rng = np.random.default_rng(first + 1000 * pop + P)
    tot = (rng.standard_normal((pop, P)) * 100.0).astype(np.float32)
    for c in range(pop):
        case = (c + first) % 6
        if case == 1:
            tot[c] = rng.integers(0, 4, P).astype(np.float32)
        elif case == 2:
            tot[c] = np.float32(rng.standard_normal() * 100.0)
        elif case in (3, 4, 5):
            tot[c, rng.integers(0, P)] = (np.float32("nan"), np.float32("inf"), np.float32("-inf"))[case - 3]
    return tot.reshape(-1)
