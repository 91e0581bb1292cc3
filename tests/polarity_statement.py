"""The polarity force library stated in numpy float64, written from the reference's
include/polarity.cuh (:13-164) -- not from this repository's include/polarity.cuh, which the device
build and the CPU oracle share.  One statement for every test that holds those forces to anything:
tests/test_model_functors_independent.py (whole Heun steps) and tests/test_polarity_pairs*.py (single
pair terms recorded inside the force kernels).

A point is (x, y, z, theta, phi); r = Xi - Xj carries the difference of the polarities in its last two
fields.  Everything is float64 except two inputs that a caller may hand over as binary32 FACTS of the
evaluation under test instead of having them recomputed:

  dist      the pair distance the kernel handed to its functor;
  quotient  r.z / dist as ONE binary32 division (quotient32), clamped to [-1, 1] before arccos.

`evaluate` returns, next to the force, its own change when that quotient moves by one binary32 ulp up
or down (clamped): no binary32 evaluation can know the quotient better, so that change is the
conditioning term of the tests' tolerance."""
import numpy as np

UNIDIRECTIONAL, BIDIRECTIONAL, BENDING, APICAL, MIGRATION = range(5)
NAMES = ("unidirectional_polarization_force", "bidirectional_polarization_force", "bending_force",
         "apical_constriction_force", "migration_force")


def pol_to_vec(theta, phi):  # polarity.cuh:13-21
    return np.array([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)])


def quotient32(r_z, dist):
    """r.z / dist as the one correctly rounded binary32 division of polarity.cuh:26."""
    with np.errstate(all="ignore"):
        return float(np.float32(r_z) / np.float32(dist))


def pt_to_pol(r, dist, quotient=None):  # polarity.cuh:23-28
    q = r[2] / dist if quotient is None else min(max(quotient, -1.0), 1.0)
    return np.arccos(q), np.arctan2(r[1], r[0])


def pol_dot_product(theta_a, phi_a, p_theta, p_phi):  # polarity.cuh:41-46
    return np.sin(theta_a) * np.sin(p_theta) * np.cos(phi_a - p_phi) + np.cos(theta_a) * np.cos(p_theta)


def unidirectional_polarization_force(theta_i, phi_i, p_theta, p_phi):  # polarity.cuh:50-60
    d_theta = np.cos(theta_i) * np.sin(p_theta) * np.cos(phi_i - p_phi) - np.sin(theta_i) * np.cos(p_theta)
    d_phi = 0.0
    if abs(np.sin(theta_i)) > 1e-10:
        d_phi = -np.sin(p_theta) * np.sin(phi_i - p_phi) / np.sin(theta_i)
    return d_theta, d_phi


def bidirectional_polarization_force(theta_i, phi_i, p_theta, p_phi):  # polarity.cuh:64-69
    prod = pol_dot_product(theta_i, phi_i, p_theta, p_phi)
    d_theta, d_phi = unidirectional_polarization_force(theta_i, phi_i, p_theta, p_phi)
    return prod * d_theta, prod * d_phi


def apical_constriction_force(Xi, r, dist, pref_angle, quotient=None):  # polarity.cuh:99-121
    pi = pol_to_vec(Xi[3], Xi[4])
    prodi = pi.dot(r[:3]) / dist + np.cos(pref_angle)
    r_hat = pt_to_pol(r, dist, quotient)
    u_theta, u_phi = unidirectional_polarization_force(Xi[3], Xi[4], *r_hat)
    dF = np.zeros(5)
    dF[3], dF[4] = -prodi * u_theta, -prodi * u_phi
    dF[:3] = -prodi / dist * pi + prodi ** 2 / dist ** 2 * r[:3]
    pj = pol_to_vec(Xi[3] - r[3], Xi[4] - r[4])  # the neighbour's polarity
    prodj = pj.dot(r[:3]) / dist - np.cos(pref_angle)
    dF[:3] += -prodj / dist * pj + prodj ** 2 / dist ** 2 * r[:3]
    return dF


def bending_force(Xi, r, dist, quotient=None):  # polarity.cuh:72-94, Xi and r = (x, y, z, theta, phi)
    pi = pol_to_vec(Xi[3], Xi[4])
    prodi = pi.dot(r[:3]) / dist
    r_hat = pt_to_pol(r, dist, quotient)
    u_theta, u_phi = unidirectional_polarization_force(Xi[3], Xi[4], *r_hat)
    dF = np.zeros(5)
    dF[3], dF[4] = -prodi * u_theta, -prodi * u_phi
    dF[:3] = -prodi / dist * pi + prodi ** 2 / dist ** 2 * r[:3]
    pj = pol_to_vec(Xi[3] - r[3], Xi[4] - r[4])  # the neighbour's polarity
    prodj = pj.dot(r[:3]) / dist
    dF[:3] += -prodj / dist * pj + prodj ** 2 / dist ** 2 * r[:3]
    return dF


def orthonormal(r3, p):  # polarity.cuh:125-131; 0 / 0 where r is parallel to p
    normal = r3 - r3.dot(p) * p
    with np.errstate(all="ignore"):
        return normal / np.sqrt(normal.dot(normal))


def migration_terms(Xi, r, dist, quotient=None):  # polarity.cuh:134-164
    """(pull, push): the two terms of the force, each None where its branch did not fire."""
    r_hat = pt_to_pol(r, dist, quotient)
    pull = push = None
    if Xi[4] != 0 or Xi[3] != 0:
        if pol_dot_product(Xi[3], Xi[4], *r_hat) <= -0.15:
            pi = pol_to_vec(Xi[3], Xi[4])
            pull = 0.6 * pi + 0.8 * orthonormal(r[:3], pi)
    theta_j, phi_j = Xi[3] - r[3], Xi[4] - r[4]
    if phi_j > 1e-10 or theta_j > 1e-10:
        if pol_dot_product(theta_j, phi_j, *r_hat) >= 0.15:
            pj = pol_to_vec(theta_j, phi_j)
            push = -(0.6 * pj + 0.8 * orthonormal(-r[:3], pj))
    return pull, push


def migration_dots(Xi, r, dist, quotient=None):
    """The two dot products migration_force compares with -0.15 and 0.15 (for the case generator's margins)."""
    r_hat = pt_to_pol(r, dist, quotient)
    return (pol_dot_product(Xi[3], Xi[4], *r_hat), pol_dot_product(Xi[3] - r[3], Xi[4] - r[4], *r_hat))


def migration_force(Xi, r, dist, quotient=None):
    dF = np.zeros(5)
    for term in migration_terms(Xi, r, dist, quotient):
        if term is not None:
            dF[:3] += term
    return dF


def decided_zeros(tag, Xi, r, dist, quotient=None):
    """The components that are 0 by a DECISION of the code, not by arithmetic: fields a function never writes,
    dF.phi behind the 1e-10 guard on sin(theta_i), migration_force where no branch fired.  (A sum that happens
    to cancel, like dF.z of bending_force on the polar axis, is arithmetic: binary32 cancels it to 0 where
    float64 leaves 1e-17.)"""
    zero = np.zeros(5, bool)
    if tag in (UNIDIRECTIONAL, BIDIRECTIONAL):
        zero[:3] = True
    if tag != MIGRATION:
        zero[4] = not abs(np.sin(Xi[3])) > 1e-10
    else:
        zero[3:] = True
        zero[:3] = all(term is None for term in migration_terms(Xi, r, dist, quotient))
    return zero


def force(tag, Xi, r, dist, pref_angle=0.0, quotient=None):
    """The library function `tag` as the recording functors of tests/native/test_polarity_pairs.cu call it: the
    two polarization forces take the partner's polarity as bending_force recovers it, Xi - r."""
    if tag in (UNIDIRECTIONAL, BIDIRECTIONAL):
        f = unidirectional_polarization_force if tag == UNIDIRECTIONAL else bidirectional_polarization_force
        dF = np.zeros(5)
        dF[3], dF[4] = f(Xi[3], Xi[4], Xi[3] - r[3], Xi[4] - r[4])
        return dF
    if tag == BENDING:
        return bending_force(Xi, r, dist, quotient)
    if tag == APICAL:
        return apical_constriction_force(Xi, r, dist, pref_angle, quotient)
    if tag == MIGRATION:
        return migration_force(Xi, r, dist, quotient)
    raise ValueError(tag)


def evaluate(tag, Xi, r, dist, pref_angle=0.0):
    """(F, c): the force with dist and the binary32 quotient as facts, and per component the larger change of
    F when the quotient moves one binary32 ulp down or up (clamped to [-1, 1]).  NaN components (the 0 / 0 of
    migration_force) give c = 0."""
    Xi, r, dist = np.asarray(Xi, np.float64), np.asarray(r, np.float64), float(dist)
    q = min(max(quotient32(r[2], dist), -1.0), 1.0)
    F = force(tag, Xi, r, dist, pref_angle, q)
    c = np.zeros(5)
    if tag >= BENDING:
        for toward in (-np.inf, np.inf):
            moved = force(tag, Xi, r, dist, pref_angle, float(np.nextafter(np.float32(q), np.float32(toward))))
            with np.errstate(invalid="ignore"):
                c = np.fmax(c, np.abs(moved - F))
    return F, np.nan_to_num(c, nan=0.0)
