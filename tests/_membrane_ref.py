"""The membrane-solve contract of include/ada_hip.h ("Membrane solve") in numpy and scipy, fp64: the sparse system, a direct solve, the norm of the
inverse that turns a residual into an error bound, the unreached components, a plain conjugate-gradient loop with the device's stopping rule, and
seamless cloning as the wrapper states it.  One image [h, w] at a time; masks are anything whose non-zero entries count."""
import numpy as np
from scipy import ndimage, sparse
from scipy.sparse.linalg import spsolve

CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])      # 4-connectivity


def masks(known, domain, shape):
    """(known & domain, domain) as bool arrays; ``domain`` None is every pixel.  known counts only inside the domain."""
    d = np.ones(shape, bool) if domain is None else np.asarray(domain) != 0
    return (np.asarray(known) != 0) & d, d


def unreached(known, domain=None):
    """bool [h, w]: the pixels of the 4-connected components of ``domain`` (known pixels included) that hold no known pixel."""
    k, d = masks(known, domain, np.shape(known))
    lab, n = ndimage.label(d, structure=CROSS)
    has = np.zeros(n + 1, bool)
    has[np.unique(lab[k])] = True
    has[0] = True      # label 0 is outside the domain: not a component
    return ~has[lab]


def system(x, known, domain=None):
    """(A csc [n, n], b [n], unknown bool [h, w]): for the n unknown pixels (in the domain, not known, reached by a known pixel), in raster order,
    deg_p u_p - sum of u_q over the unknown neighbours = sum of x_q over the known neighbours.  An edge that leaves the image or the domain does not
    exist.  x under a pixel that is not known is never read.  The unreached pixels are no unknowns: the solve says nothing about them."""
    x = np.asarray(x, np.float64)
    h, w = x.shape
    k, d = masks(known, domain, x.shape)
    unk = d & ~k & ~unreached(k, d)
    n = int(unk.sum())
    num = np.full((h, w), -1, np.int64)
    num[unk] = np.arange(n)
    data = np.where(k, x, 0.0)      # a select: NaN under a pixel that is not known stays out
    deg = np.zeros((h, w))
    b = np.zeros((h, w))
    rows, cols = [], []
    for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        src = (slice(max(dy, 0), h + min(dy, 0)), slice(max(dx, 0), w + min(dx, 0)))      # the neighbour q = p + (dy, dx)
        dst = (slice(max(-dy, 0), h + min(-dy, 0)), slice(max(-dx, 0), w + min(-dx, 0)))     # the pixel p
        edge = unk[dst] & d[src]
        deg[dst] += edge
        b[dst] += np.where(edge & k[src], data[src], 0.0)
        both = edge & unk[src]
        rows.append(num[dst][both])
        cols.append(num[src][both])
    r, c = np.concatenate(rows), np.concatenate(cols)
    A = sparse.coo_matrix((np.concatenate([deg[unk], -np.ones(r.size)]), (np.concatenate([np.arange(n), r]), np.concatenate([np.arange(n), c]))),
                          shape=(n, n)).tocsc()
    return A, b[unk], unk


def solve_direct(A, b):
    if A.shape[0] == 0:
        return np.zeros(0)
    return np.atleast_1d(spsolve(A, b))


def kappa(A):
    """max (A^-1 1) = the infinity norm of A^-1: the inverse of an M-matrix has no negative entry, so its largest row sum is attained on the ones."""
    if A.shape[0] == 0:
        return 0.0
    return float(np.max(solve_direct(A, np.ones(A.shape[0]))))


def residual(A, b, u):
    """max |b - A u| (0 for an empty system)."""
    return float(np.max(np.abs(b - A @ u))) if b.size else 0.0


def cg(A, b, u0, tol, cap):
    """Plain conjugate gradients with the device's stopping rule: stop once the recurrence residual's max norm is <= tol, once p.Ap <= 0 or after
    ``cap`` steps.  Returns (u, steps taken)."""
    u = np.array(u0, np.float64)
    r = b - A @ u
    rr = float(r @ r)
    p = r.copy()
    steps = 0
    while steps < cap and b.size and np.max(np.abs(r)) > tol:
        q = A @ p
        pq = float(p @ q)
        if not pq > 0.0:
            break
        alpha = rr / pq
        u += alpha * p
        r -= alpha * q
        rr_new = float(r @ r)
        p = r + (rr_new / rr) * p
        rr = rr_new
        steps += 1
    return u, steps


def fill(x, known, domain=None, empty=0.0):
    """fp64 [h, w]: the direct solve on the unknowns, ``empty`` on the unreached pixels, x itself everywhere else."""
    A, b, unk = system(x, known, domain)
    out = np.asarray(x, np.float64).copy()
    out[unk] = solve_direct(A, b)
    k, d = masks(known, domain, out.shape)
    out[unreached(k, d) & ~k] = empty
    return out


def seamless(src, dst, mask, known=None, domain=None):
    """fp64 [h, w]: src + the harmonic extension of dst - src from the known pixels (default: every pixel outside ``mask``) over the domain (default
    mask | known, and always met with it); dst on the known pixels and outside mask | known; src where no known pixel reaches."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    m = np.asarray(mask) != 0
    k = ~m if known is None else np.asarray(known) != 0
    d = (m | k) if domain is None else ((np.asarray(domain) != 0) & (m | k))
    k = k & d
    c = fill(np.where(k, dst - src, 0.0), k, d, empty=0.0)
    return np.where(d & ~k, src + c, dst)
