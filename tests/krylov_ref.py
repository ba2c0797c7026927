"""NumPy restatements of the reference's BiCGStab, CR, steepest descent and minimal residual (pyamg/krylov/_bicgstab.py, _cr.py,
_steepest_descent.py, _minimal_residual.py) under criteria 'rr', as MultilevelSolver.solve(accel=...) runs them: x0 = 0,
A = the fine-level operator (anything with @), M = a function applying the preconditioner.  Same operations in the same order as
the reference; the test side never imports the product.

Each returns (x, info, residuals)."""
from __future__ import annotations

import warnings

import numpy as np


def _norm(v):
    return np.sqrt(np.inner(v.conj(), v).real)


def bicgstab(A, b, M, tol=1e-5, maxiter=None):
    b = np.ravel(b)
    x = np.zeros_like(b)
    if maxiter is None:
        maxiter = len(x) + 5
    r = b - A @ x
    normr = _norm(r)
    res = [normr]
    normb = _norm(b)
    if normb == 0.0:
        normb = 1.0
    rtol = tol * normb
    if normr < rtol:
        return x, 0, res
    rstar = r.copy()
    p = r.copy()
    rrstarOld = np.inner(rstar.conjugate(), r)
    it = 0
    with np.errstate(divide="ignore", invalid="ignore"):
        while True:
            Mp = M(p)
            AMp = A @ Mp
            alpha = rrstarOld / np.inner(rstar.conjugate(), AMp)
            s = r - alpha * AMp
            Ms = M(s)
            AMs = A @ Ms
            omega = np.inner(AMs.conjugate(), s) / np.inner(AMs.conjugate(), AMs)
            x = x + alpha * Mp + omega * Ms
            r = s - omega * AMs
            rrstarNew = np.inner(rstar.conjugate(), r)
            beta = (rrstarNew / rrstarOld) * (alpha / omega)
            rrstarOld = rrstarNew
            p = r + beta * (p - omega * AMp)
            it += 1
            normr = _norm(r)
            res.append(normr)
            if normr < rtol:
                return x, 0, res
            if it == maxiter:
                return x, it, res


def cr(A, b, M, tol=1e-5, maxiter=None):
    b = np.ravel(b)
    x = np.zeros_like(b)
    if maxiter is None:
        maxiter = int(1.3 * len(b)) + 2
    r = b - A @ x
    z = M(r)
    p = z.copy()
    normr = np.linalg.norm(r)
    res = [normr]
    normb = _norm(b)
    if normb == 0.0:
        normb = 1.0
    rtol = tol * normb
    if normr < rtol:
        return x, 0, res
    Az = A @ z
    rAz = np.inner(r.conjugate(), Az)
    Ap = A @ p
    it = 0
    while True:
        rAz_old = rAz
        alpha = rAz / np.inner(Ap.conjugate(), Ap)
        x += alpha * p
        if np.mod(it, 8) and it > 0:
            r -= alpha * Ap
        else:
            r = b - A @ x
        z = M(r)
        Az = A @ z
        rAz = np.inner(r.conjugate(), Az)
        beta = rAz / rAz_old
        p *= beta
        p += z
        Ap *= beta
        Ap += Az
        it += 1
        zz = np.inner(z.conjugate(), z)
        normr = np.linalg.norm(r)
        res.append(normr)
        if normr < rtol:
            return x, 0, res
        if zz == 0.0:
            warnings.warn("\nSingular preconditioner detected in CR, ceasing iterations\n")
            return x, -1, res
        if it == maxiter:
            return x, it, res


def steepest_descent(A, b, M, tol=1e-5, maxiter=None):
    b = np.ravel(b)
    x = np.zeros_like(b)
    if maxiter is None:
        maxiter = len(b)
    r = b - A @ x
    z = M(r)
    rz = np.inner(r.conjugate(), z)
    res = [np.linalg.norm(r)]
    normb = _norm(b)
    if normb == 0.0:
        normb = 1.0
    rtol = tol * normb
    it = 0
    while True:
        q = A @ z
        zAz = np.inner(z.conjugate(), q)
        if zAz < 0.0:
            warnings.warn("\nIndefinite matrix detected in steepest descent, aborting\n")
            return x, -1, res
        alpha = rz / zAz
        x = x + alpha * z
        it += 1
        if np.mod(it, 50) and it > 0:        # the reference's test, inverted as it is there: recompute except every 50th
            r = b - A @ x
        else:
            r = r - alpha * q
        z = M(r)
        rz = np.inner(r.conjugate(), z)
        if rz < 0.0:
            warnings.warn("\nIndefinite preconditioner detected in steepest descent, stopping.\n")
            return x, -1, res
        normr = _norm(r)
        res.append(normr)
        if normr < rtol:
            return x, 0, res
        if rz == 0.0:
            warnings.warn("\nSingular preconditioner detected in steepest descent, stopping.\n")
            return x, -1, res
        if it == maxiter:
            return x, it, res


def minimal_residual(A, b, M, tol=1e-5, maxiter=None):
    b = np.ravel(b)
    x = np.zeros_like(b)
    if maxiter is None:
        maxiter = int(1.3 * len(b)) + 2
    r = b - A @ x
    z = M(r)
    normr = _norm(z)
    res = [normr]
    normb = _norm(b)
    normMb = 1.0 if normb == 0.0 else _norm(M(b))
    if normr < tol * normMb:
        return x, 0, res
    it = 0
    while True:
        p = M(A @ z)
        pz = np.inner(p.conjugate(), z)
        if pz < 0.0:
            warnings.warn("\nIndefinite matrix detected in minimal residual, stopping.\n")
            return x, -1, res
        alpha = pz / np.inner(p.conjugate(), p)
        x = x + alpha * z
        it += 1
        if np.mod(it, 50) and it > 0:        # as steepest descent: two preconditioner applications on most iterations
            r = b - A @ x
            z = M(r)
        else:
            z = z - alpha * p
        normr = _norm(z)
        res.append(normr)
        if normr < tol * normMb:
            return x, 0, res
        if it == maxiter:
            return x, it, res


METHODS = {"bicgstab": bicgstab, "cr": cr, "steepest_descent": steepest_descent, "minimal_residual": minimal_residual}
