"""TEST INFRASTRUCTURE ONLY -- float64 closed-form oracle for the Lie-group kernels.

The reference's dependency (princeton-vl/lietorch 0.2) is absent from /root/reference (empty submodule) and the
reference holds no test or golden vector at this boundary => PARITY UNPINNED against lietorch itself.  The oracle is
the matrix exponential/logarithm of the 4x4 twist (scipy.linalg.expm/logm, fp64) with the conventions visible at the
reference call sites: data [t, q_xyzw(, s)], tangent [tau, phi(, sigma)], retr(a) = exp(a) * X."""
import numpy as np
from scipy.linalg import expm, logm
from scipy.spatial.transform import Rotation


def hat(phi):
    x, y, z = phi
    return np.array([[0, -z, y], [z, 0, -x], [-y, x, 0.0]])


def twist_matrix(group, a):
    a = np.asarray(a, np.float64)
    M = np.zeros((4, 4))
    if group == 0:
        M[:3, :3] = hat(a[:3])
    else:
        M[:3, :3] = hat(a[3:6]) + (a[6] if group == 2 else 0.0) * np.eye(3)
        M[:3, 3] = a[:3]
    return M


def exp_matrix(group, a):
    return expm(twist_matrix(group, a))


def data_to_matrix(group, d):
    d = np.asarray(d, np.float64)
    M = np.eye(4)
    if group == 0:
        M[:3, :3] = Rotation.from_quat(d[:4]).as_matrix()
    else:
        s = d[7] if group == 2 else 1.0
        M[:3, :3] = s * Rotation.from_quat(d[3:7]).as_matrix()
        M[:3, 3] = d[:3]
    return M


def matrix_to_data(group, M):
    M = np.asarray(M, np.float64)
    if group == 0:
        return Rotation.from_matrix(M[:3, :3]).as_quat()
    s = np.cbrt(np.linalg.det(M[:3, :3])) if group == 2 else 1.0
    q = Rotation.from_matrix(M[:3, :3] / s).as_quat()
    d = np.concatenate([M[:3, 3], q])
    return np.concatenate([d, [s]]) if group == 2 else d


def vee(group, L):
    """tangent vector of a 4x4 algebra element (inverse of twist_matrix)"""
    phi = np.array([L[2, 1], L[0, 2], L[1, 0]])
    if group == 0:
        return phi
    tau = L[:3, 3]
    if group == 1:
        return np.concatenate([tau, phi])
    return np.concatenate([tau, phi, [np.trace(L[:3, :3]) / 3.0]])


def log_tangent(group, M):
    return vee(group, np.real(logm(M)))


def adjoint_matrix(group, M, eps=1e-6):
    """numerical Ad: X exp(a) X^-1 = exp(Ad a)  =>  column j = d/da_j log(X exp(a) X^-1) at 0 (central differences)"""
    n = {0: 3, 1: 6, 2: 7}[group]
    Ad = np.zeros((n, n))
    Mi = np.linalg.inv(M)
    for j in range(n):
        e = np.zeros(n)
        e[j] = eps
        p = log_tangent(group, M @ exp_matrix(group, e) @ Mi)
        m = log_tangent(group, M @ exp_matrix(group, -e) @ Mi)
        Ad[:, j] = (p - m) / (2 * eps)
    return Ad


# ---- vectorised / logm-free twins for sweeps of thousands of points (logm costs milliseconds per 4x4); tests/test_lie_bands_gpu.py checks
# each against the function it stands for
def exp_matrix_batch(group, A):
    """exp_matrix of every row of A [N, tangent dim] -> [N, 4, 4] (one batched scipy expm)"""
    A = np.asarray(A, np.float64)
    return expm(np.stack([twist_matrix(group, a) for a in A]))


def matrix_to_data_batch(group, M):
    """matrix_to_data of every matrix of M [N, 4, 4], with the quaternion sign fixed to w >= 0"""
    M = np.asarray(M, np.float64)
    s = np.cbrt(np.linalg.det(M[:, :3, :3])) if group == 2 else np.ones(len(M))
    q = Rotation.from_matrix(M[:, :3, :3] / s[:, None, None]).as_quat()
    q = q * np.where(q[:, 3:4] < 0, -1.0, 1.0)
    if group == 0:
        return q
    d = np.concatenate([M[:, :3, 3], q], 1)
    return np.concatenate([d, s[:, None]], 1) if group == 2 else d


def adjoint_matrix_exact(group, M):
    """Ad without differences: X a^ X^-1 = (Ad a)^  =>  column j = vee(X e_j^ X^-1)"""
    n = {0: 3, 1: 6, 2: 7}[group]
    Mi = np.linalg.inv(M)
    return np.stack([vee(group, M @ twist_matrix(group, np.eye(n)[j]) @ Mi) for j in range(n)], 1)
