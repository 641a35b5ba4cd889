"""Warp meshes from a camera calibration (host only, numpy, float64).

`rectify_mesh` computes the node grid `frontend.Warp` / pislam_warp_create take (include/pislam_hip.h) from a pinhole
calibration with OpenCV's distortion model, after cv::initUndistortRectifyMap: for each node, the position in the
distorted camera image that the output (undistorted, rectified) pixel comes from.  Nothing here touches the device.
"""
from __future__ import annotations

import numpy as np

NODE_LO, NODE_HI = -(1 << 23), (1 << 23) - 1          # the node range of pislam_warp_create


def mesh_dims(width: int, height: int, log_cell: int):
    """(mesh_w, mesh_h) of pislam_warp_mesh_dims, without the library."""
    if not (1 <= width <= 4096 and 1 <= height <= 4096 and 0 <= log_cell <= 6):
        raise ValueError("need 1 <= width, height <= 4096 and 0 <= log_cell <= 6")
    return ((width - 1) >> log_cell) + 2, ((height - 1) >> log_cell) + 2


def distort_points(K, dist, x, y):
    """Normalised pinhole coordinates (x, y) -> pixel coordinates in the distorted image: the radial (k1 k2 k3 over
    k4 k5 k6) and tangential (p1 p2) model in OpenCV's coefficient order k1 k2 p1 p2 [k3 [k4 k5 k6]]."""
    K = np.asarray(K, np.float64)
    d = np.zeros(8)
    dist = np.asarray(dist, np.float64).ravel()
    if dist.size not in (4, 5, 8):
        raise ValueError("dist takes 4, 5 or 8 coefficients (k1 k2 p1 p2 [k3 [k4 k5 k6]])")
    d[:dist.size] = dist
    k1, k2, p1, p2, k3, k4, k5, k6 = d
    r2 = x * x + y * y
    radial = (1 + r2 * (k1 + r2 * (k2 + r2 * k3))) / (1 + r2 * (k4 + r2 * (k5 + r2 * k6)))
    xd = x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * radial + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]


def source_position(K, dist, R, P, u, v):
    """Float64 source position (in pixels of the distorted image) of output pixel (u, v); arrays broadcast."""
    K = np.asarray(K, np.float64)
    R = np.eye(3) if R is None else np.asarray(R, np.float64)
    P = K if P is None else np.asarray(P, np.float64)
    if K.shape != (3, 3) or R.shape != (3, 3) or P.shape not in ((3, 3), (3, 4)):
        raise ValueError("K and R are 3 x 3, P is 3 x 3 or 3 x 4")
    u, v = np.broadcast_arrays(np.asarray(u, np.float64), np.asarray(v, np.float64))
    ray = np.stack([(u - P[0, 2]) / P[0, 0], (v - P[1, 2]) / P[1, 1], np.ones_like(u)])
    X, Y, Z = np.tensordot(np.linalg.inv(R), ray, axes=1)
    return distort_points(K, dist, X / Z, Y / Z)


def rectify_mesh(K, dist, R=None, P=None, size=None, log_cell: int = 3):
    """(mesh_x, mesh_y) int32 [mesh_h][mesh_w] for an output of size = (width, height): node (j, i) = the Q8 source
    position of output pixel (i * C, j * C), C = 1 << log_cell, rounded to nearest and clipped to the node range.
    K: 3 x 3 camera matrix of the distorted image; dist: 4, 5 or 8 distortion coefficients in OpenCV order;
    R: rectifying rotation (default identity); P: new camera matrix, 3 x 3 or 3 x 4 (default K)."""
    if size is None:
        raise ValueError("size = (width, height) of the output is required")
    width, height = int(size[0]), int(size[1])
    mw, mh = mesh_dims(width, height, log_cell)
    C = 1 << log_cell
    u, v = np.meshgrid(np.arange(mw, dtype=np.float64) * C, np.arange(mh, dtype=np.float64) * C)
    sx, sy = source_position(K, dist, R, P, u, v)
    q8 = lambda s: np.clip(np.rint(256.0 * np.nan_to_num(s, nan=0.0, posinf=1e12, neginf=-1e12)), NODE_LO, NODE_HI).astype(np.int32)
    return q8(sx), q8(sy)


def interpolate_mesh(mesh, width: int, height: int, log_cell: int):
    """The Q8 source coordinate of every output pixel (int64 [height][width]) by the header's integer statement —
    for checks and accuracy figures on the host."""
    m = np.asarray(mesh, np.int64)
    C = 1 << log_cell
    x, y = np.meshgrid(np.arange(width), np.arange(height))
    i, fx, j, fy = x >> log_cell, x & (C - 1), y >> log_cell, y & (C - 1)
    a = (m[j, i] * (C - fx) + m[j, i + 1] * fx + (C >> 1)) >> log_cell
    b = (m[j + 1, i] * (C - fx) + m[j + 1, i + 1] * fx + (C >> 1)) >> log_cell
    return (a * (C - fy) + b * fy + (C >> 1)) >> log_cell
