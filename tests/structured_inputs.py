"""Structured and extreme transform inputs with closed-form coset-LDE outputs.  Pure Python and numpy: no GPU, no oracle.

Everything is a Montgomery WORD (uint32 < P).  The transforms are linear, so the kernels transform the words themselves with
canonical twiddles; an "extreme" input is an extreme word, and every closed form below is stated on words with the CANONICAL
shift (a shift is passed the way the entry points take it, as a Montgomery word, and converted here).

Evaluation-domain families (a column of height n = 2^log_h on the subgroup <w>):
    const(v)             v everywhere                       -> v on every LDE row
    delta(r, v)          v at row r                         -> (v / n) * sum_k (x / w^r)^k
    alternating(v, u)    v on even rows, u on odd rows      -> u + ((v - u) / 2) * (1 + x^(n/2))
    block(m, v)          v for i < 2^m                      -> (v / n) (x^n - 1) * sum_{r < 2^m} 1 / (x / w^r - 1)
    comb(m, v)           v where i = 0 (mod 2^m)            -> (v / 2^m) * sum_{u < 2^m} x^(u n / 2^m)
Coefficient-domain families (the natural-order coefficient column c whose SCALED coefficients c'[k] = c[k] (shift g^j)^k,
g the generator of the LDE domain of n << added points, are v on a set and 0 elsewhere):
    coeff_block(m, v, shift, j, added)   c'[k] = v for k < 2^m           -> v * sum_{k < 2^m} (g^(i - j))^k at LDE row i
    coeff_comb(m, v, shift, j, added)    c'[k] = v for k = 0 (mod 2^m)   -> v * sum_t (g^(i - j))^(t 2^m)
Rows are natural-order rows of the LDE: x_i = shift * g^i."""
import numpy as np

P = 0x78000001
R = 1 << 32
RINV = pow(R, P - 2, P)
GEN = 31
AMPL = [P - 1, 1, (P - 1) // 2, (P + 1) // 2]
EVAL_FAMILIES = ("const", "delta", "alternating", "block", "comb")
COEFF_FAMILIES = ("coeff_block", "coeff_comb")
_PU = np.uint64(P)


def to_word(canonical):
    return canonical % P * R % P


def from_word(word):
    return word * RINV % P


def inv(x):
    return pow(x % P, P - 2, P)


def two_adic_generator(bits):
    return pow(pow(GEN, 15, P), 1 << (27 - bits), P)


def _mulmod(a, b):
    """numpy uint64 arrays (or scalars) of values < P"""
    return (a * b) % _PU


def geometric(q, length):
    """[q^0, q^1, .., q^(length-1)] mod P as uint64, by doubling"""
    out = np.ones(1, dtype=np.uint64)
    step = q % P
    while out.size < length:
        out = np.concatenate([out, _mulmod(out, np.uint64(step))])
        step = step * step % P
    return out[:length]


def batch_inverse(a):
    """Inverses mod P of a 1-D uint64 array of nonzero residues (Montgomery's trick on 256 interleaved chains)."""
    n = a.size
    if n == 0:
        return a.copy()
    K = 256
    rows = -(-n // K)
    pad = np.ones(rows * K, dtype=np.uint64)
    pad[:n] = a
    m = pad.reshape(K, rows)  # chain along axis 0: each step is one vector operation over `rows` lanes
    pre = np.empty_like(m)
    pre[0] = m[0]
    for i in range(1, K):
        pre[i] = _mulmod(pre[i - 1], m[i])
    tot_inv = np.array([inv(int(t)) for t in pre[K - 1]], dtype=np.uint64)
    out = np.empty_like(m)
    for i in range(K - 1, 0, -1):
        out[i] = _mulmod(tot_inv, pre[i - 1])
        tot_inv = _mulmod(tot_inv, m[i])
    out[0] = tot_inv
    return out.reshape(-1)[:n]


# ---------------------------------------------------------------- generators
def const(log_h, v):
    return np.full(1 << log_h, v, dtype=np.uint32)


def delta(log_h, r, v):
    x = np.zeros(1 << log_h, dtype=np.uint32)
    x[r] = v
    return x


def alternating(log_h, v, u=0):
    x = np.full(1 << log_h, u, dtype=np.uint32)
    x[::2] = v
    return x


def block(log_h, m, v):
    x = np.zeros(1 << log_h, dtype=np.uint32)
    x[:1 << m] = v
    return x


def comb(log_h, m, v):
    x = np.zeros(1 << log_h, dtype=np.uint32)
    x[::1 << m] = v
    return x


def delta_rows(log_h, rng):
    """{0, 1, n/2, n-1} plus one seeded random row"""
    n = 1 << log_h
    return sorted({0, 1 % n, n // 2, n - 1, int(rng.integers(0, n))})


def _coset_point_inv(log_h, shift, j, added):
    """1 / (shift g^j), canonical"""
    g = two_adic_generator(log_h + added)
    return inv(from_word(shift) * pow(g, j, P))


def coeff_block(log_h, m, v, shift, j, added):
    c = np.zeros(1 << log_h, dtype=np.uint32)
    q = _coset_point_inv(log_h, shift, j, added)
    c[:1 << m] = _mulmod(geometric(q, 1 << m), np.uint64(v))
    return c


def coeff_comb(log_h, m, v, shift, j, added):
    c = np.zeros(1 << log_h, dtype=np.uint32)
    q = _coset_point_inv(log_h, shift, j, added)
    c[::1 << m] = _mulmod(geometric(pow(q, 1 << m, P), 1 << (log_h - m)), np.uint64(v))
    return c


GENERATORS = {"const": const, "delta": delta, "alternating": alternating, "block": block, "comb": comb,
              "coeff_block": coeff_block, "coeff_comb": coeff_comb}


def generate(family, log_h, **params):
    """The family's input column: evaluations for the evaluation-domain families, COEFFICIENTS for the coefficient-domain ones
    (their evaluation-domain input is the dft of this column)."""
    return GENERATORS[family](log_h, **params)


# ---------------------------------------------------------------- closed forms
def _geom_sum(y, n):
    """sum_{t < n} y^t"""
    y %= P
    if y == 1:
        return n % P
    return (pow(y, n, P) - 1) * inv(y - 1) % P


_WINV_POWERS = {}


def _arc_sum(log_h, start, length, xs, v):
    """Interpolant of (v on rows [start, start + length) of the subgroup of order n, 0 elsewhere) at the points xs: the sum of
    the Lagrange basis polynomials of those rows, (v / n) (x^n - 1) sum_r 1 / (x / w^r - 1)."""
    n = 1 << log_h
    if length == 0:
        return [0] * len(xs)
    if log_h not in _WINV_POWERS or _WINV_POWERS[log_h].size < start + length:
        _WINV_POWERS.clear()  # one table at a time: 8 MiB at 2^20
        _WINV_POWERS[log_h] = geometric(inv(two_adic_generator(log_h)), start + length)
    wr = _WINV_POWERS[log_h][start:start + length]
    ninv = inv(n)
    out = []
    per = max(1, (1 << 22) // length)
    for c0 in range(0, len(xs), per):
        chunk = xs[c0:c0 + per]
        d = (_mulmod(np.array(chunk, dtype=np.uint64)[:, None], wr[None, :]) + np.uint64(P - 1)) % _PU  # x / w^r - 1
        hit = ~d.all(axis=1)  # x is w^r for an r inside the arc
        d[d == 0] = 1
        sums = batch_inverse(d.reshape(-1)).reshape(d.shape).sum(axis=1, dtype=np.uint64)  # < 2^22 * 2^31
        for x, h, sm in zip(chunk, hit, sums):
            xn = pow(x, n, P)
            out.append(v if h else 0 if xn == 1 else v * ninv % P * (xn - 1) % P * (int(sm) % P) % P)
    return out


def closed_form(family, params, rows):
    """Expected coset-LDE output words of the family's column at the natural-order LDE rows `rows`.
    params: log_h, added, shift (Montgomery word) and the family's own parameters (v, r, u, m, j)."""
    log_h, added = params["log_h"], params["added"]
    n = 1 << log_h
    g = two_adic_generator(log_h + added)
    s = from_word(params["shift"])
    v = params.get("v", 0)
    rows = [int(i) for i in rows]
    xs = [s * pow(g, i, P) % P for i in rows]
    if family == "const":
        out = [v] * len(rows)
    elif family == "delta":
        wr_inv = inv(pow(two_adic_generator(log_h), params["r"], P))
        out = [v * inv(n) % P * _geom_sum(x * wr_inv, n) % P for x in xs]
    elif family == "alternating":
        u = params.get("u", 0)
        if log_h == 0:
            out = [v] * len(rows)
        else:
            out = [(u + (v - u) * inv(2) % P * (1 + pow(x, n // 2, P))) % P for x in xs]
    elif family == "comb":
        m = params["m"]
        out = [v * inv(1 << m) % P * _geom_sum(pow(x, n >> m, P), 1 << m) % P for x in xs]
    elif family == "block":
        length = 1 << params["m"]
        if length <= n // 2:
            out = _arc_sum(log_h, 0, length, xs, v)
        else:  # the constant minus the complementary arc: at most n / 2 terms per row
            out = [(v - t) % P for t in _arc_sum(log_h, length, n - length, xs, v)]
    elif family in COEFF_FAMILIES:
        m, j, order = params["m"], params["j"], n << added
        rho = [pow(g, (i - j) % order, P) for i in rows]
        if family == "coeff_block":
            out = [v * _geom_sum(y, 1 << m) % P for y in rho]
        else:
            out = [v * _geom_sum(pow(y, 1 << m, P), n >> m) % P for y in rho]
    else:
        raise KeyError(family)
    return np.array(out, dtype=np.uint32)


def generator_params(family, params):
    """the subset of closed_form's params that the family's generator takes"""
    keys = {"const": ("v",), "delta": ("r", "v"), "alternating": ("v", "u"), "block": ("m", "v"), "comb": ("m", "v"),
            "coeff_block": ("m", "v", "shift", "j", "added"), "coeff_comb": ("m", "v", "shift", "j", "added")}[family]
    return {k: params[k] for k in keys if k in params}


def sample_rows(log_h, added, rng, count):
    """`count` seeded rows plus 0, 1, n-1, n and the last row of the LDE (natural order)"""
    n, total = 1 << log_h, (1 << log_h) << added
    fixed = {0, 1 % total, n - 1, n % total, total - 1}
    return sorted(fixed | {int(i) for i in rng.integers(0, total, size=count)})


def bit_reverse_index(rows, bits):
    """positions of natural-order rows in a bit-reversed matrix of 2^bits rows"""
    out = np.zeros(len(rows), dtype=np.int64)
    r = np.asarray(rows, dtype=np.int64)
    for b in range(bits):
        out |= ((r >> b) & 1) << (bits - 1 - b)
    return out


# ---------------------------------------------------------------- packing
def pack(columns, width, rng):
    """Puts the pattern columns side by side in one (n, width) matrix at seeded positions and fills the remaining columns with
    seeded random words.  Returns (matrix, positions): positions[k] is the matrix column of columns[k]."""
    assert 0 < len(columns) <= width
    n = len(columns[0])
    pos = sorted(int(p) for p in rng.permutation(width)[:len(columns)])
    mat = np.empty((n, width), dtype=np.uint32)
    fill = [c for c in range(width) if c not in set(pos)]
    if fill:
        mat[:, fill] = rng.integers(0, P, size=(n, len(fill)), dtype=np.uint32)
    for p, col in zip(pos, columns):
        mat[:, p] = col
    return mat, pos


# ---------------------------------------------------------------- case lists
def _clip(ms, log_h):
    return list(range(log_h + 1)) if ms is None else sorted({m for m in ms if 0 <= m <= log_h})


def eval_templates(log_h, rng, ms=None, ampl=(P - 1,), const_ampl=tuple(AMPL) + (0,), delta_ampl=None):
    """[(family, own params)] of the evaluation-domain families: const at const_ampl, the deltas (amplitudes of `delta_ampl`,
    default `ampl`, in turn), alternating and block / comb at every m of `ms` (default 0..log_h) at every amplitude of `ampl`."""
    delta_ampl = delta_ampl or ampl
    ms = _clip(ms, log_h)
    out = [("const", {"v": v}) for v in const_ampl]
    out += [("delta", {"r": r, "v": delta_ampl[k % len(delta_ampl)]}) for k, r in enumerate(delta_rows(log_h, rng))]
    for v in ampl:
        out.append(("alternating", {"v": v, "u": 0}))
        out += [(f, {"m": m, "v": v}) for f in ("block", "comb") for m in ms]
    return out


def coeff_templates(log_h, ms=None, ampl=(P - 1,), js=("first", "last")):
    """[(family, own params)] of the coefficient-domain families; j is "first" (coset 0) or "last" (coset 2^added - 1) until
    bind() knows the blowup."""
    return [(f, {"m": m, "v": v, "j": j}) for v in ampl for f in COEFF_FAMILIES for m in _clip(ms, log_h) for j in js]


def bind(template, log_h, added, shift):
    """(family, own params) -> (family, closed_form's params) for one transform"""
    fam, own = template
    prm = dict(own, log_h=log_h, added=added, shift=shift)
    if prm.get("j") in ("first", "last"):
        prm["j"] = 0 if prm["j"] == "first" else (1 << added) - 1
    return fam, prm


def family_cases(log_h, added, shift, rng, ms=None, ampl=(P - 1,), coeff_ampl=(P - 1,), const_ampl=tuple(AMPL) + (0,),
                 coeff_ms=None):
    """[(family, params)] over every family for one transform (params are closed_form's); coefficient families at
    j in {0, 2^added - 1}."""
    tmpl = eval_templates(log_h, rng, ms, ampl, const_ampl)
    tmpl += coeff_templates(log_h, ms if coeff_ms is None else coeff_ms, coeff_ampl, ("first", "last") if added else ("first",))
    return [bind(t, log_h, added, shift) for t in tmpl]


def column_of(family, params):
    return generate(family, params["log_h"], **generator_params(family, params))
