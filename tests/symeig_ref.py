"""Float64 numpy statement of the device eigenvalue solve (mtrl_amd/csrc/symeig.hip), the
case matrices and the error bar.  Nothing here looks at a kernel's output.  Shared by tests/test_symeig_cpu.py,
tests/test_gpu_symeig.py and tests/test_gpu_network_eigvals.py.

Statement, for a symmetric A of order r:
  tridiag   for k = 0 .. r - 3, x = A[k+1:, k]: if x[1:] is all zero there is no reflection (e_k = x_0); else
            alpha = -sign(x_0) |x| (sign(0) = +1), e_k = alpha, v = (1, x[1:] / (x_0 - alpha)),
            tau = (alpha - x_0) / alpha, p = tau A[k+1:, k+1:] v, w = p - (tau / 2)(p^T v) v,
            A[k+1:, k+1:] -= v w^T + w v^T.  d_k = a_kk as the reduction reaches it; e_{r-2} = a_{r-1, r-2}.
  eigvals   eigenvalue j (ascending) by bisection on the Sturm count of LAPACK's dlaebz,
            q_i = d_i - x - e_{i-1}^2 / q_{i-1}, |q| <= pivmin replaced by -pivmin, count = #(q_i <= 0), from
            the Gershgorin interval widened by 2 r 2^-52 |T| + 2 pivmin, HALVINGS halvings whatever the data.
            |T| = 0: exact zeros.  A non-finite entry of A (flag bit 0) or of d, e, e^2 (bit 1): all NaN.
numpy sums in another order than the device and contracts nothing; the device contracts nothing either but
adds row sums lane by lane and through trees.

The bar: |lam_j - ref_j| <= C_EIG * r * 2^-52 * max|ref|, compared sorted.  C_EIG is four times the worst ratio
err / (r 2^-52 max|ref|) of this statement over `cpu_cases()` (the factor four: the device's other summation
order), rounded up to a power of two; tests/test_symeig_cpu.py holds the statement to C_EIG / 4 and prints the
measured worst ratio.
"""

from __future__ import annotations

import numpy as np

HALVINGS = 64
U52 = 2.0 ** -52
SAFMIN = 2.0 ** -1022
C_EIG = 4.0  # measured worst ratio of the statement over cpu_cases(): 0.95, at r = 1


# ------------------------------------------------------------------ statement
def tridiag(A, drop_last_step=False, full_tau=False):
    """(d, e) of the Householder reduction.  The two switches plant faults for the bar's own test."""
    A = np.array(A, np.float64)
    r = A.shape[0]
    d, e = np.empty(r), np.empty(max(r - 1, 0))
    last = r - 3 - (1 if drop_last_step else 0)
    for k in range(r):
        d[k] = A[k, k]
        m = r - k - 1
        if m == 0:
            break
        x = A[k + 1:, k].copy()
        tail = float(np.sum(x[1:] * x[1:]))
        if m < 2 or k > last or tail == 0.0:
            e[k] = x[0]
            continue
        with np.errstate(all="ignore"):
            alpha = -np.copysign(np.sqrt(x[0] * x[0] + tail), x[0])
            tau = (alpha - x[0]) / alpha
            v = x / (x[0] - alpha)
            v[0] = 1.0
            e[k] = alpha
            T = A[k + 1:, k + 1:]
            p = tau * (T @ v)
            c = (tau if full_tau else 0.5 * tau) * float(p @ v)
            w = p - c * v
            T -= np.outer(v, w) + np.outer(w, v)
    return d, e


def sturm_counts(d, e, x, pivmin):
    """Eigenvalues of tridiag(d, e) below each x (vector)."""
    with np.errstate(all="ignore"):
        q = d[0] - x
        q = np.where(np.abs(q) <= pivmin, -pivmin, q)
        cnt = (q <= 0).astype(np.int64)
        for i in range(1, d.size):
            q = d[i] - x - e[i - 1] * e[i - 1] / q
            q = np.where(np.abs(q) <= pivmin, -pivmin, q)
            cnt += q <= 0
    return cnt


def tridiag_eigvals(d, e, halvings=HALVINGS, count_offset=0):
    """(lam ascending, flag) of the symmetric tridiagonal matrix."""
    d, e = np.asarray(d, np.float64), np.asarray(e, np.float64)
    r = d.size
    with np.errstate(all="ignore"):
        ea = np.abs(e)
        rad = np.concatenate([[0.0], ea]) + np.concatenate([ea, [0.0]])
        e2 = ea * ea
        if not (np.all(np.isfinite(d)) and np.all(np.isfinite(rad)) and np.all(np.isfinite(e2))):
            return np.full(r, np.nan), 2
        gl, gu = float(np.min(d - rad)), float(np.max(d + rad))
    tnorm = max(abs(gl), abs(gu))
    if tnorm == 0.0:
        return np.zeros(r), 0
    pivmin = SAFMIN * max(1.0, float(np.max(e2)) if e2.size else 0.0)
    wide = 2.0 * tnorm * U52 * r + 2.0 * pivmin
    lo, hi = np.full(r, gl - wide), np.full(r, gu + wide)
    need = np.arange(r) + 1 + count_offset
    for _ in range(halvings):
        mid = 0.5 * lo + 0.5 * hi
        left = sturm_counts(d, e, mid, pivmin) >= need
        hi = np.where(left, mid, hi)
        lo = np.where(left, lo, mid)
    return 0.5 * lo + 0.5 * hi, 0


def sym_eigvals(A, **faults):
    """(lam ascending, flag, d, e) of one symmetric matrix by the statement above."""
    A = np.asarray(A, np.float64)
    r = A.shape[0]
    t_faults = {k: v for k, v in faults.items() if k in ("drop_last_step", "full_tau")}
    b_faults = {k: v for k, v in faults.items() if k in ("halvings", "count_offset")}
    with np.errstate(all="ignore"):
        d, e = tridiag(A, **t_faults)
    if not np.all(np.isfinite(A)):
        return np.full(r, np.nan), 1, d, e
    lam, flag = tridiag_eigvals(d, e, **b_faults)
    return lam, flag, d, e


def bar(r, ref, c=C_EIG):
    ref = np.asarray(ref, np.float64)
    return c * r * U52 * (float(np.max(np.abs(ref))) if ref.size else 0.0)


def ratio(lam, ref):
    """max |sort(lam) - sort(ref)| / (r 2^-52 max|ref|); 0 when both are all zero."""
    lam, ref = np.sort(np.asarray(lam, np.float64)), np.sort(np.asarray(ref, np.float64))
    scale = lam.size * U52 * float(np.max(np.abs(ref)))
    err = float(np.max(np.abs(lam - ref)))
    return 0.0 if err == 0.0 else err / scale


# ------------------------------------------------------------------ case matrices
def relu_acts(M, W, seed):
    rng = np.random.default_rng(seed)
    return np.maximum(rng.standard_normal((M, W)) + 0.3, 0).astype(np.float32)


def gram(H):
    """The smaller Gram of H in float64 from float32-exact entries, exactly symmetric."""
    H = np.asarray(H, np.float32).astype(np.float64)
    G = H.T @ H if H.shape[1] <= H.shape[0] else H @ H.T
    return np.triu(G) + np.triu(G, 1).T


def gram_full(r, seed):
    return gram(relu_acts(r + 7, r, seed))


def gram_collapsed(r, rank, seed):
    """Rows repeat `rank` prototypes: the Gram has rank <= `rank` (a collapsed representation)."""
    H = relu_acts(rank, r, seed)
    return gram(H[np.arange(r + 7) % rank])


def gram_zero_columns(r, seed):
    """Planted dead neurons: zero rows and columns, so the reduction meets tau = 0 midway."""
    H = relu_acts(r + 7, r, seed)
    dead = np.random.default_rng(seed + 1).choice(r, max(1, r // 4), replace=False)
    H[:, dead] = 0.0
    if r >= 3:
        H[:, 1] = 0.0  # and one in the very first column step
    return gram(H)


def diagonal(r, seed):
    v = np.random.default_rng(seed).uniform(-3, 5, r)
    return np.diag(v), np.sort(v)


def graded_diagonal(r):
    v = 10.0 ** np.linspace(-12, 12, r) if r > 1 else np.array([1e12])
    return np.diag(v), np.sort(v)


def rank_one(r, seed):
    u = np.random.default_rng(seed).standard_normal(r)
    lam = np.zeros(r)
    lam[-1] = float(u @ u)
    return np.outer(u, u), lam


def toeplitz(r):
    A = 2.0 * np.eye(r) - np.eye(r, k=1) - np.eye(r, k=-1)
    return A, np.sort(2.0 - 2.0 * np.cos(np.arange(1, r + 1) * np.pi / (r + 1)))


def block_copies(r, seed):
    """Two or three copies of one random symmetric block on the diagonal, shuffled by a permutation: every
    eigenvalue of the block repeats.  Order r exactly (the last block is padded by a zero block)."""
    rng = np.random.default_rng(seed)
    b = max(1, r // 3)
    B = rng.standard_normal((b, b))
    B = B + B.T
    A = np.zeros((r, r))
    copies = r // b
    for c in range(copies):
        A[c * b:(c + 1) * b, c * b:(c + 1) * b] = B
    perm = rng.permutation(r)
    A = A[np.ix_(perm, perm)]
    lam = np.sort(np.concatenate([np.tile(np.linalg.eigvalsh(B), copies), np.zeros(r - copies * b)]))
    return A, lam


def wilkinson21():
    """W21+: diagonal |i - 10|, off-diagonal 1; its large eigenvalues come in pairs that agree to many digits."""
    A = np.diag(np.abs(np.arange(21) - 10.0)) + np.eye(21, k=1) + np.eye(21, k=-1)
    return A, None


def mixed(M, seed):
    """A dense orthogonal similarity of M: the same spectrum with no structure left."""
    r = M.shape[0]
    Q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((r, r)))
    A = Q @ M @ Q.T
    return np.triu(A) + np.triu(A, 1).T


def cases(sizes):
    """[(name, A, closed-form spectrum or None)] over the given orders."""
    out = []
    for r in sizes:
        out.append((f"gram_full r={r}", gram_full(r, 10 + r), None))
        out.append((f"gram_zero_columns r={r}", gram_zero_columns(r, 20 + r), None))
        A, lam = diagonal(r, 30 + r)
        out.append((f"diagonal r={r}", A, lam))
        A, lam = graded_diagonal(r)
        out.append((f"graded_diagonal r={r}", A, lam))
        A, lam = rank_one(r, 40 + r)
        out.append((f"rank_one r={r}", A, lam))
        A, lam = toeplitz(r)
        out.append((f"toeplitz r={r}", A, lam))
        out.append((f"toeplitz_mixed r={r}", mixed(A, 50 + r), lam))
        A, lam = block_copies(r, 60 + r)
        out.append((f"block_copies r={r}", A, lam))
        out.append((f"zero r={r}", np.zeros((r, r)), np.zeros(r)))
    for r, rank in ((65, 2), (65, 6), (130, 2), (130, 6)):
        if r <= max(sizes):
            out.append((f"gram_collapsed r={r} rank={rank}", gram_collapsed(r, rank, 70 + r + rank), None))
    A, _ = wilkinson21()
    out.append(("wilkinson21", A, None))
    out.append(("wilkinson21_mixed", mixed(A, 99), None))
    return out


CPU_SIZES = (1, 2, 3, 4, 5, 17, 48, 65)
GPU_SIZES = (1, 2, 3, 4, 5, 17, 63, 64, 65, 130, 257)


def cpu_cases():
    return cases(CPU_SIZES)
