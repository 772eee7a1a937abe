"""NumPy restatement of the reference's interp (src/util.jl:17-43) and of the particle step built on it — the yardstick of
tests/test_interp_cpu.py, tests/test_gpu_interp.py, tests/test_gpu_probes.py and tests/test_gpu_tracers.py.

interp(x, arr, T): every statement of :17-43 in arrays of type T.  T = float32 keeps the written order — clamp, x + 1.5, floor, y = x − i,
then the 2^D corners in CartesianIndices order (first dimension fastest), each weight the product over d taken left to right, `s += arr[J]*w`
as a multiply and an add — which is the order the device kernel uses (the reference's @fastmath @simd fixes none).  T = float64 is the same
formula on the same float32 inputs, the value the error bound is measured from.

Arrays are numpy arrays indexed [x, y(, z)(, component)]; points are (n, D)."""
import numpy as np


def _interp_scalar(x, arr, T):
    """_interp(_interp_clamp(x, size(arr)), arr)   :17-18, :29-43 for (n, D) points x (already of type T)"""
    n, D = x.shape
    y = np.empty((n, D), dtype=T)
    i0 = np.empty((n, D), dtype=np.int64)
    for d in range(D):
        c = np.clip(x[:, d], T(0), T(arr.shape[d] - 2))       # clamp(x[d], 0, sz[d]-2) :18
        c = (c + T(1.5)).astype(T)                             # x .+ 1.5f0 :31
        fl = np.floor(c)
        y[:, d] = (c - fl).astype(T)
        i0[:, d] = fl.astype(np.int64) - 1                     # Julia index i -> 0-based
    s = np.zeros(n, dtype=T)
    a = arr.astype(T)
    for q in range(1 << D):                                    # J in I:I+oneunit(I): first dimension fastest :38
        w = None
        idx = []
        for d in range(D):
            up = (q >> d) & 1
            f = y[:, d] if up else (T(1) - y[:, d]).astype(T)  # ifelse(J.I==I.I, 1-y, y) :39
            w = f if w is None else (w * f).astype(T)          # prod, left to right
            idx.append(i0[:, d] + up)
        s = (s + (a[tuple(idx)] * w).astype(T)).astype(T)      # s += arr[J]*weight :40
    return s


def interp(x, arr, T=np.float32):
    """interp.(x, Ref(arr)): arr with x.shape[1] dimensions -> (n,); with one more (the staggered vector array) -> (n, D), component i queried at
    x + ½·eᵢ (:20-25).  The points are taken as float32 numbers whatever T is."""
    x32 = np.asarray(x, dtype=np.float32)
    n, D = x32.shape
    if arr.ndim == D:
        return _interp_scalar(x32.astype(T), arr, T)
    assert arr.ndim == D + 1 and arr.shape[-1] == D
    out = np.empty((n, D), dtype=T)
    for i in range(D):
        xs = x32.astype(T).copy()
        xs[:, i] = (xs[:, i] + T(0.5)).astype(T)               # shift(i) :23
        out[:, i] = _interp_scalar(xs, arr[..., i], T)
    return out


def advect(x, u0, u1, dt, perdir=(), T=np.float32):
    """one step of a particle swarm, as the pathline extension's update does with the current flow: returns (x_new, x_prev);
    x* = x⁰ + Δt·u⁰(x⁰);  x = x⁰ + ½Δt·(u⁰(x⁰) + u¹(x*));  coordinates of a periodic direction j (1-based, as perdir) wrapped into [0, N_j)"""
    x0 = np.asarray(x, dtype=np.float32).astype(T)
    dt = T(np.float32(dt))
    v0 = _interp_T(x0, u0, T)
    xs = (x0 + (dt * v0).astype(T)).astype(T)
    v1 = _interp_T(xs, u1, T)
    xn = (x0 + ((T(0.5) * dt) * (v0 + v1).astype(T)).astype(T)).astype(T)
    for j in perdir:
        N = T(u0.shape[j - 1] - 2)
        w = (xn[:, j - 1] - (N * np.floor((xn[:, j - 1] / N).astype(T))).astype(T)).astype(T)
        w[~(w >= 0) | (w >= N)] = 0
        xn[:, j - 1] = w
    return xn, x0.copy()


def _interp_T(x, arr, T):
    """interp of a vector array at points that are already numbers of type T (in the float64 chain of advect x* is not rounded to float32)"""
    n, D = x.shape
    out = np.empty((n, D), dtype=T)
    for i in range(D):
        xs = x.copy()
        xs[:, i] = xs[:, i] + T(0.5)
        out[:, i] = _interp_scalar(xs, arr[..., i], T)
    return out


def loc_array(shape, i, comp):
    """a[I] = loc(i,I)[comp] on a grid of `shape` (Julia: loc(i,I) = I − 1.5 − ½δᵢ, I 1-based; i = 0: the cell centre)   src/core.jl:177"""
    idx = np.indices(shape)[comp].astype(np.float32)
    return (idx + np.float32(1) - np.float32(1.5) - np.float32(0.5 if i == comp + 1 else 0.0)).astype(np.float32)


def known_answer_arrays():
    """a (8×8×2, a[I,i] = loc(i,I)[i]) and b (8×8, b[I] = loc(0,I)[1]) of the reference's test/test_util.jl:3-14, in Float32"""
    a = np.stack([loc_array((8, 8), 1, 0), loc_array((8, 8), 2, 1)], axis=-1)
    b = loc_array((8, 8), 0, 0)
    return np.asfortranarray(a), np.asfortranarray(b)


# (point, array name, expected) — test/test_util.jl:3-14
KNOWN = [((2.5, 1.0), "a", (2.5, 1.0)), ((3.5, 3.0), "a", (3.5, 3.0)), ((-1.0, 4.0), "a", (-0.5, 4.0)), ((2.5, 1.0), "b", 2.5), ((10.0, 10.0), "b", 6.0)]


def bound(ref32, ref64, arr):
    """the issue's bound: |device − ref64| ≤ 4·max_points|ref32 − ref64|, with a floor of 4·eps32·max|arr|"""
    return max(4.0 * float(np.abs(ref32.astype(np.float64) - ref64).max(initial=0.0)), 4.0 * float(np.finfo(np.float32).eps) * float(np.abs(arr).max()))
