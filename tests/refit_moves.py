"""The moves the refit tests apply to a scene's triangles (reference layout, leaf order): float64 arithmetic, float32 out."""
import numpy as np


def rotated(tri, norm, deg=7.0, axis=(0.3, 1.0, 0.2)):
    """rigid rotation of the whole scene about its centre, normals / tangents / bitangents rotated with it"""
    a = np.asarray(axis, np.float64); a /= np.linalg.norm(a)
    th = np.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    M = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    v = tri.reshape(-1, 3).astype(np.float64)
    c = (v.min(0) + v.max(0)) / 2
    out = ((v - c) @ M.T + c).astype(np.float32).reshape(-1)
    n = (norm.reshape(-1, 3).astype(np.float64) @ M.T).astype(np.float32).reshape(-1)
    return out, n


def sine(tri, amp):
    """sine-wave deformation: y += amp * size * sin(3 pi x / size), size = the scene's longest side"""
    v = tri.reshape(-1, 3).astype(np.float64).copy()
    size = float((v.max(0) - v.min(0)).max())
    v[:, 1] += amp * size * np.sin(3 * np.pi * v[:, 0] / size)
    return v.astype(np.float32).reshape(-1)
