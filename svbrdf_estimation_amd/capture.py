"""Captured photographs onto the patch grid, and renderings into a perspective camera: the step between a camera image and
``losses.PhotoLoss`` / ``fitting.PhotoFit``.

The photo losses take photographs as ``[B,S,3,H,W]`` float32, linear, on the patch's orthographic pixel grid, with an optional
confidence plane per photo.  A captured photograph is a perspective image of the patch, usually 8-bit and gamma encoded, much
larger than the grid, with clipped highlights and pixels outside the patch.  ``rectify`` takes it there in ONE kernel launch
(svbrdf_rectify_photos, csrc/svbrdf_capture.hip): a 3x3 homography per photo, bilinear taps, the decode of 8-bit codes
through a 256-entry table, and the ``{0,1}`` weights, all bit for bit a numpy float32 restatement (tests/capture_checks.py).

    corners = ...                                                # the patch's four corners in the photo, in pixels
    M = capture.patch_homography(corners, (256, 256))            # destination pixel -> source pixel
    photos, weights = capture.rectify(images_u8, M, 256, lut=capture.gamma_lut(), clip=(5, 250), samples=2)
    loss = losses.PhotoLoss(renderers.LocalRenderer())(maps, photos, scenes, weights)

``to_perspective`` is the other direction, the reference's ``OrthoToPerspectiveMapping.apply`` (renderers.py:106-173, there a
cv2 warp): the same kernel with the inverse matrix.  ``camera_corners`` / ``camera_from_corners`` go between a camera
position and the corners it sees, for a first guess of the pose that ``PhotoLoss``'s scene gradient then refines.

Conventions.  A matrix maps a DESTINATION pixel index ``(x, y, 1)`` to SOURCE pixel-index coordinates; integer coordinates
are pixel centres (cv2's convention).  That matches the patch grid: ``linspace(-1, 1, W)`` puts pixel 0's centre on the patch
edge, so the patch corners are the centres of the grid's corner pixels, ``(0, 0)``, ``(0, H-1)``, ``(W-1, H-1)``, ``(W-1, 0)``
in the reference's corner order top-left, bottom-left, bottom-right, top-right.  (The reference's ``get_homography`` stretches
the ``W`` x ``H`` image over ``[0, W] x [0, H]`` instead, half a pixel off at each edge; what is kept here is the camera.)

Gradients.  ``rectify`` is differentiable towards its MATRICES: if ``matrices`` is a tensor that requires grad, the returned
values carry a ``grad_fn`` whose backward is ONE more launch (svbrdf_rectify_photos_grad_matrices,
csrc/svbrdf_capture_grad.hip), so a registration can be refined photometrically -- ``corner_matrices`` makes the matrices
from the four corner positions differentiably, and an optimiser holds the eight corner coordinates:

    corners = torch.tensor(clicked, dtype=torch.float64, requires_grad=True)          # [P,4,2], source pixels
    photos, weights = capture.rectify(images_u8, capture.corner_matrices(corners, 256), 256, lut=capture.gamma_lut())
    ((photos - rendering).abs() * weights[:, None]).sum().div(weights.sum()).backward()        # corners.grad

No gradient flows towards the images, the weights are piecewise constant (marked non-differentiable), and there is no double
backward.  There is no CPU path.

Lens distortion.  A homography is exact only for a pinhole camera; a hand-held phone bends straight lines by several pixels
towards the frame's edge.  ``rectify(..., lens=)`` takes OpenCV's ``fx, fy, cx, cy, k1, k2, p1, p2, k3`` per photo
(``lens_table``; ``pinhole_lens`` gives this module's camera with zero coefficients) and applies the FORWARD model, ideal
pixel -> distorted pixel, inside the same one launch (svbrdf_rectify_photos_lens, csrc/svbrdf_capture_lens.hip): a
closed-form polynomial between the homography and the taps, no iteration.  The matrices then map to IDEAL coordinates.
Corners clicked in a photograph are DISTORTED coordinates, while ``patch_homography`` / ``corner_matrices`` need ideal ones:

    ideal = capture.undistort_points(clicked, lens)                  # Newton on the host, float64
    M = capture.patch_homography(ideal, (256, 256))
    photos, weights = capture.rectify(images_u8, M, 256, lut=capture.gamma_lut(), lens=lens)

If ``matrices`` and/or ``lens`` require grad the backward is ONE launch (svbrdf_rectify_photos_lens_grad,
csrc/svbrdf_capture_lens_grad.hip) that returns both gradients, the matrices' through the lens's Jacobian.  Refine ONE
coefficient per stage (k1 beside the corners): k1 and k2 trade off against each other on a patch that covers the middle
of the frame.  ``to_perspective`` stays pinhole: rendering INTO a distorted camera needs the inverse map per pixel.
"""
import math

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _native

F32_PLANAR, U8_INTERLEAVED = 0, 1        # SVBRDF_RECTIFY_F32_PLANAR / SVBRDF_RECTIFY_U8_INTERLEAVED of include/svbrdf_hip.h
_PATCH_CORNERS = np.array([[-1.0, 1.0], [-1.0, -1.0], [1.0, -1.0], [1.0, 1.0]])    # top-left, bottom-left, bottom-right, top-right


# ------------------------------------------------------------------------------------------------ lookup tables

def gamma_lut(gamma=2.2):
    """float32 [256]: code / 255 to the power ``gamma`` (``utils.gamma_decode``'s rule on an 8-bit code), computed on the host
    in float64 and rounded once"""
    codes = np.arange(256, dtype=np.float64) / 255.0
    return torch.from_numpy(np.power(codes, float(gamma)).astype(np.float32))


def srgb_lut():
    """float32 [256]: the sRGB electro-optical transfer function (IEC 61966-2-1) on an 8-bit code: c / 12.92 up to 0.04045,
    ((c + 0.055) / 1.055) ** 2.4 above; float64 on the host, rounded once"""
    c = np.arange(256, dtype=np.float64) / 255.0
    lin = np.where(c <= 0.04045, c / 12.92, np.power((c + 0.055) / 1.055, 2.4))
    return torch.from_numpy(lin.astype(np.float32))


# ------------------------------------------------------------------------------------------------ homographies

def _size(size):
    """(H, W) from an int or a pair"""
    if isinstance(size, (int, np.integer)):
        return int(size), int(size)
    H, W = size
    return int(H), int(W)


def _homography(src, dst):
    """float64 [3,3] with h8 = 1 that sends the four points ``src`` [4,2] to ``dst`` [4,2]: the 8x8 linear system"""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    if src.shape != (4, 2) or dst.shape != (4, 2):
        raise ValueError("a homography needs four (x, y) points on each side")
    A, b = np.zeros((8, 8)), np.zeros(8)
    for k, ((x, y), (u, v)) in enumerate(zip(src, dst)):
        A[2 * k] = (x, y, 1.0, 0.0, 0.0, 0.0, -u * x, -u * y)
        A[2 * k + 1] = (0.0, 0.0, 0.0, x, y, 1.0, -v * x, -v * y)
        b[2 * k], b[2 * k + 1] = u, v
    return np.append(np.linalg.solve(A, b), 1.0).reshape(3, 3)


def patch_homography(corners, size, dtype=np.float32):
    """The matrix ``rectify`` takes for a photograph in which the patch's corners sit at the source-pixel positions
    ``corners`` [4,2] (x, y), in the reference's order top-left, bottom-left, bottom-right, top-right: it sends the
    destination pixel centres (0, 0), (0, H-1), (W-1, H-1), (W-1, 0) of a ``size`` = (H, W) grid onto them.  One float64 8x8
    solve, rounded to ``dtype`` once at the end (float32: what the kernel reads; float64: the solve itself)."""
    H, W = _size(size)
    if H < 2 or W < 2:
        raise ValueError("a grid of %dx%d has no four distinct corner centres" % (H, W))
    corners = np.asarray(corners, np.float64)
    if corners.shape == (4, 3):         # homogeneous, as the reference's target_points
        corners = corners[:, :2] / corners[:, 2:3]
    grid = np.array([[0.0, 0.0], [0.0, H - 1.0], [W - 1.0, H - 1.0], [W - 1.0, 0.0]])
    return _homography(grid, corners).astype(dtype)


def corner_matrices(corners, size):
    """``patch_homography`` for torch tensors, differentiable: ``corners`` ``[...,4,2]`` (x, y) in source pixels, in the
    reference's order top-left, bottom-left, bottom-right, top-right -> float64 ``[...,3,3]`` (m8 = 1) on the corners'
    device, through one batched ``torch.linalg.solve`` of the same 8x8 system.  The eight corner coordinates are what an
    optimiser should hold: they are in pixels and well conditioned; the nine matrix entries are neither, and scaling a
    matrix changes nothing (``rectify``'s gradient is orthogonal to it)."""
    H, W = _size(size)
    if H < 2 or W < 2:
        raise ValueError("a grid of %dx%d has no four distinct corner centres" % (H, W))
    if not isinstance(corners, torch.Tensor) or corners.shape[-2:] != (4, 2):
        raise ValueError("corners must be a tensor [...,4,2]")
    c = corners.to(torch.float64)
    lead = c.shape[:-2]
    grid = torch.tensor([[0.0, 0.0], [0.0, H - 1.0], [W - 1.0, H - 1.0], [W - 1.0, 0.0]], dtype=torch.float64, device=c.device)
    x, y = grid[:, 0].expand(lead + (4,)), grid[:, 1].expand(lead + (4,))
    u, v = c[..., 0], c[..., 1]
    one, zero = torch.ones_like(u), torch.zeros_like(u)
    rows_u = torch.stack((x, y, one, zero, zero, zero, -u * x, -u * y), dim=-1)         # [...,4,8]
    rows_v = torch.stack((zero, zero, zero, x, y, one, -v * x, -v * y), dim=-1)
    A = torch.stack((rows_u, rows_v), dim=-2).reshape(lead + (8, 8))                    # rows 2k, 2k + 1 as _homography's
    b = c.reshape(lead + (8, 1))
    h = torch.linalg.solve(A, b)[..., 0]
    return torch.cat((h, torch.ones_like(h[..., :1])), dim=-1).reshape(lead + (3, 3))


def _camera(camera_pos, sensor_size):
    """(K, R, C): intrinsics, world-to-camera rotation (rows = the camera's axes in world coordinates) and centre of the
    reference's look-at camera (renderers.py:106-156), float64"""
    C = np.asarray(camera_pos, np.float64).reshape(3)
    dist = np.linalg.norm(C)
    if not dist > 0.0:
        raise ValueError("the camera cannot sit in the origin it looks at")
    cz = -C / dist                                          # the principal axis points at the origin
    cx = np.cross(cz, np.array([0.0, 0.0, 1.0]))            # up is the patch's normal
    n = np.linalg.norm(cx)
    cx = np.array([1.0, 0.0, 0.0]) if n == 0.0 else cx / n  # straight overhead (or below): up and axis are parallel
    cy = np.cross(cz, cx)
    R = np.stack((cx, cy, cz))
    sw, sh = float(sensor_size[0]), float(sensor_size[1])
    K = np.array([[sw / 2.0, 0.0, sw / 2.0], [0.0, sw / 2.0, sh / 2.0], [0.0, 0.0, 1.0]])   # focal length: half the width
    return K, R, C


def camera_corners(camera_pos, sensor_size):
    """float64 [4,2]: where a camera at ``camera_pos`` that looks at the origin sees the patch corners (-1,1,0), (-1,-1,0),
    (1,-1,0), (1,1,0) on a sensor of ``sensor_size`` = (width, height) pixels -- the reference's
    ``OrthoToPerspectiveMapping(camera, sensor_size).target_points`` without the homogeneous column.  The principal axis
    points at the origin, up is +z (x = (1, 0, 0) straight overhead), the focal length is width / 2 and the principal point
    the sensor's centre."""
    K, R, C = _camera(camera_pos, sensor_size)
    P = K @ np.concatenate((R, (-R @ C)[:, None]), axis=1)
    world = np.concatenate((_PATCH_CORNERS, np.zeros((4, 1)), np.ones((4, 1))), axis=1)
    img = (P @ world.T).T
    return img[:, :2] / img[:, 2:3]


def camera_from_corners(corners, sensor_size):
    """Inverse of ``camera_corners``: the camera position, float64 [3], from the four corner positions by planar pose --
    the homography G from patch coordinates (X, Y) to pixels is K [r1 r2 t] up to scale, so K^-1 G gives two columns of
    the rotation and the translation, and the centre is -R^T t.  A first guess for the pose (``tools/fit_photos.py
    --captured --fit-pose`` refines it); exact for corners that ``camera_corners`` made."""
    corners = np.asarray(corners, np.float64)
    if corners.shape == (4, 3):
        corners = corners[:, :2] / corners[:, 2:3]
    G = _homography(_PATCH_CORNERS, corners)
    sw, sh = float(sensor_size[0]), float(sensor_size[1])
    Kinv = np.array([[2.0 / sw, 0.0, -1.0], [0.0, 2.0 / sw, -sh / sw], [0.0, 0.0, 1.0]])
    A = Kinv @ G
    scale = 2.0 / (np.linalg.norm(A[:, 0]) + np.linalg.norm(A[:, 1]))
    if A[2, 2] < 0.0:               # the patch lies in front of the camera: t_z > 0
        scale = -scale
    r1, r2, t = A[:, 0] * scale, A[:, 1] * scale, A[:, 2] * scale
    R = np.stack((r1, r2, np.cross(r1, r2)), axis=1)
    return -R.T @ t


def perspective_matrix(camera_pos, sensor_size, size, t=1.0, dtype=np.float32):
    """The matrix ``to_perspective`` hands the kernel: the INVERSE of ``t G + (1 - t) I`` with G the mapping from the pixels
    of a ``size`` = (H, W) rendering to the sensor of the camera (``patch_homography(camera_corners(...), size)`` in float64)
    -- the reference's ``apply`` blends its homography with the identity the same way.  t = 0: the identity."""
    G = patch_homography(camera_corners(camera_pos, sensor_size), size, dtype=np.float64)
    blend = float(t) * G + (1.0 - float(t)) * np.eye(3)
    return np.linalg.inv(blend).astype(dtype)


# ------------------------------------------------------------------------------------------------ lens distortion

def lens_table(fx, fy, cx, cy, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0):
    """float32 [9]: ``fx, fy, cx, cy, k1, k2, p1, p2, k3`` -- OpenCV's camera matrix entries and its distortion vector in
    OpenCV's order -- as ``rectify(..., lens=)`` takes it"""
    return torch.tensor([fx, fy, cx, cy, k1, k2, p1, p2, k3], dtype=torch.float64).to(torch.float32)


def pinhole_lens(sensor_size):
    """float32 [9]: the intrinsics of this module's camera (``_camera``: focal length = width / 2, principal point at the
    sensor's centre (width / 2, height / 2)) with zero distortion coefficients, for ``sensor_size`` = (width, height)"""
    K, _, _ = _camera((0.0, 0.0, 1.0), sensor_size)
    return lens_table(K[0, 0], K[1, 1], K[0, 2], K[1, 2])


def _lens_f64(lens):
    lens = np.asarray(lens.detach().cpu() if isinstance(lens, torch.Tensor) else lens, np.float64)
    if lens.shape != (9,):
        raise ValueError("lens must be [9]: fx, fy, cx, cy, k1, k2, p1, p2, k3")
    return lens


def _distort_normalised(xn, yn, lens):
    """(xd, yd, mono, jxx, jxy, jyy) of the polynomial at normalised coordinates, float64"""
    _, _, _, _, k1, k2, p1, p2, k3 = lens
    xx, yy, xy = xn * xn, yn * yn, xn * yn
    r2 = xx + yy
    rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    mono = 1.0 + r2 * (3.0 * k1 + r2 * (5.0 * k2 + r2 * (7.0 * k3)))
    xd = xn * rad + (p1 * 2.0 * xy + p2 * (r2 + 2.0 * xx))
    yd = yn * rad + (p1 * (r2 + 2.0 * yy) + p2 * 2.0 * xy)
    q = k1 + r2 * (2.0 * k2 + 3.0 * k3 * r2)
    jxx = rad + 2.0 * xx * q + 2.0 * p1 * yn + 6.0 * p2 * xn
    jxy = 2.0 * xy * q + 2.0 * p1 * xn + 2.0 * p2 * yn
    jyy = rad + 2.0 * yy * q + 6.0 * p1 * yn + 2.0 * p2 * xn
    return xd, yd, mono, jxx, jxy, jyy


def distort_points(points, lens):
    """Ideal (pinhole) pixel coordinates ``[...,2]`` (x, y) -> where the lens puts them, numpy float64 on the host: OpenCV's
    forward model, xn = (x - cx) / fx, r2 = xn^2 + yn^2, xd = xn (1 + k1 r2 + k2 r2^2 + k3 r2^3) + 2 p1 xn yn + p2 (r2 +
    2 xn^2), yd likewise with p1 (r2 + 2 yn^2) + 2 p2 xn yn, x' = xd fx + cx."""
    lens = _lens_f64(lens)
    pts = np.asarray(points, np.float64)
    if pts.shape[-1:] != (2,):
        raise ValueError("points must be [...,2]")
    fx, fy, cx, cy = lens[:4]
    xd, yd = _distort_normalised((pts[..., 0] - cx) / fx, (pts[..., 1] - cy) / fy, lens)[:2]
    return np.stack((xd * fx + cx, yd * fy + cy), axis=-1)


def undistort_points(points, lens):
    """The inverse of ``distort_points``: distorted pixel coordinates ``[...,2]`` (corners clicked in a photograph) -> ideal
    ones (what ``patch_homography`` / ``corner_matrices`` need), numpy float64 on the host.  Newton iteration with the
    polynomial's 2x2 Jacobian from the point itself; it stops at a step below 1e-12 px or after 50 iterations, and raises
    ``ValueError`` if it did not converge or ended where the radial map has folded back (mono <= 0)."""
    lens = _lens_f64(lens)
    pts = np.asarray(points, np.float64)
    if pts.shape[-1:] != (2,):
        raise ValueError("points must be [...,2]")
    fx, fy, cx, cy = lens[:4]
    tx, ty = (pts[..., 0] - cx) / fx, (pts[..., 1] - cy) / fy
    xn, yn = tx.copy(), ty.copy()
    converged = False
    with np.errstate(all="ignore"):
        for _ in range(50):
            xd, yd, _, jxx, jxy, jyy = _distort_normalised(xn, yn, lens)
            ex, ey = xd - tx, yd - ty
            det = jxx * jyy - jxy * jxy
            dx, dy = (jyy * ex - jxy * ey) / det, (jxx * ey - jxy * ex) / det
            xn, yn = xn - dx, yn - dy
            step = np.max(np.hypot(dx * fx, dy * fy)) if pts.size else 0.0
            if not np.isfinite(step):
                break
            if step < 1e-12:
                converged = True
                break
        mono = _distort_normalised(xn, yn, lens)[2]
    if not converged or not np.all(mono > 0.0):
        raise ValueError("undistort_points did not converge inside the lens's monotonic range")
    return np.stack((xn * fx + cx, yn * fy + cy), axis=-1)


# ------------------------------------------------------------------------------------------------ the launch

def _as_tensor(t):
    return t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(t)))


def _device_rows(rows, lead, device, shape_error, lead_error):
    """``rows`` (tensor, [...,9] with the photos' leading dimensions, or one [9] for all) -> contiguous float32 [P,9] on
    ``device``; the two messages are the caller's"""
    P = int(np.prod(lead)) if lead else 1
    if rows.shape[-1:] != (9,):
        raise ValueError(shape_error % (tuple(rows.shape),))
    if rows.dim() == 1:
        rows = rows.expand(P, 9)
    elif tuple(rows.shape[:-1]) != tuple(lead):
        raise ValueError(lead_error % (tuple(rows.shape), tuple(lead)))
    return rows.reshape(P, 9).to(device=device, dtype=torch.float32).contiguous()


def _device_matrices(matrices, lead, device):
    """``matrices`` (tensor or array, [...,3,3] or [...,9] with the photos' leading dimensions, or one [3,3] for all) ->
    contiguous float32 [P,9] on ``device``"""
    m = _as_tensor(matrices)
    if m.shape[-2:] == (3, 3):
        m = m.reshape(m.shape[:-2] + (9,))
    return _device_rows(m, lead, device, "matrices must be [...,3,3] or [...,9], got %s",
                        "matrices %s do not match the photos' leading dimensions %s")


def _device_lens(lens, lead, device):
    """``lens`` (tensor or array, [...,9] with the photos' leading dimensions, or one [9] for all) -> contiguous float32 [P,9]
    on ``device``"""
    return _device_rows(_as_tensor(lens), lead, device, "lens must be [...,9] (fx, fy, cx, cy, k1, k2, p1, p2, k3), got %s",
                        "lens %s does not match the photos' leading dimensions %s")


def rectify(photos, matrices, size, lut=None, clip=None, samples=1, want_weights=True, lens=None):
    """Source photographs through one homography each onto a ``size`` = (H, W) (or int) grid, ONE launch.

    ``photos``: a device tensor, uint8 ``[...,Hs,Ws,3]`` (interleaved, what an image decoder returns) or float32
    ``[...,3,Hs,Ws]``; the leading dimensions ``[B,S]`` or ``[P]`` (or none) are kept.  ``matrices``: ``[...,3,3]`` with the
    same leading dimensions, or one ``[3,3]`` for all; tensor or array, on any device (see the module's conventions).
    If ``matrices`` is a tensor that requires grad, the values carry a ``grad_fn``: its backward is one launch of
    svbrdf_rectify_photos_grad_matrices and returns the gradient in the shape, dtype and device of ``matrices`` (one matrix
    for all: the sum over the photos).  It is the gradient of the values with the tap cell and the weights held constant.
    There is no gradient towards ``photos``, the weights are non-differentiable, and there is no double backward.
    ``lut``: float32 [256], required for uint8 sources (``gamma_lut()``, ``srgb_lut()``, a camera response) and refused for
    float ones.  ``clip`` = (lo, hi): a tap with a channel <= lo or >= hi is invalid (codes for uint8 sources, values for
    float ones; None: off).  ``samples``: k of the k x k sub-samples per pixel, 1, 2 or 4.
    -> (photos ``[...,3,H,W]``, weights ``[...,H,W]``) float32 on the source's device: what ``PhotoLoss.forward(..., weights)``
    and ``PhotoFit.step`` accept.  A pixel with any invalid sub-sample -- outside the source, behind the horizon, a NaN or
    clipped tap -- has values 0 and weight 0, every other weight 1.  ``want_weights=False``: -> (photos, None), the weight
    plane is never written.
    ``lens``: None (a pinhole camera: the launch above), or ``[...,9]`` with the photos' leading dimensions, or one ``[9]`` for
    all (``lens_table``): the lens's forward model is applied between the homography and the taps inside the one launch
    (svbrdf_rectify_photos_lens), and ``matrices`` map to IDEAL source coordinates (``undistort_points`` takes clicked
    corners there).  A sub-sample where the radial map has folded back is invalid.  If ``matrices`` and/or ``lens`` require
    grad, the backward is one launch of svbrdf_rectify_photos_lens_grad and returns the gradient in the shape, dtype and
    device of each input that asked (a shared matrix or a shared lens: the sum over the photos in float64)."""
    if not isinstance(photos, torch.Tensor):
        raise TypeError("photos must be a torch.Tensor")
    if not photos.is_cuda:
        raise _native.NativeLibraryError(
            "photos are on %s: the MI355X engine only computes on a ROCm device (no CPU fallback)" % photos.device)
    if samples not in (1, 2, 4):
        raise ValueError("samples must be 1, 2 or 4, got %r" % (samples,))
    Hd, Wd = _size(size)
    if Hd < 1 or Wd < 1:
        raise ValueError("size must be at least 1x1")
    if photos.dtype == torch.uint8:
        if photos.dim() < 3 or photos.shape[-1] != 3:
            raise ValueError("uint8 photos must be [...,Hs,Ws,3], got %s" % (tuple(photos.shape),))
        fmt, lead, (Hs, Ws) = U8_INTERLEAVED, tuple(photos.shape[:-3]), photos.shape[-3:-1]
        if lut is None:
            raise ValueError("uint8 photos need a lut (capture.gamma_lut(), capture.srgb_lut() or a camera response)")
        lut = torch.as_tensor(lut)
        if lut.dtype != torch.float32 or tuple(lut.shape) != (256,):
            raise ValueError("lut must be float32 [256]")
        lut = lut.to(photos.device).contiguous()
    elif photos.dtype == torch.float32:
        if photos.dim() < 3 or photos.shape[-3] != 3:
            raise ValueError("float32 photos must be [...,3,Hs,Ws], got %s" % (tuple(photos.shape),))
        fmt, lead, (Hs, Ws) = F32_PLANAR, tuple(photos.shape[:-3]), photos.shape[-2:]
        if lut is not None:
            raise ValueError("float32 photos are used as they are: no lut")
    else:
        raise TypeError("photos must be uint8 [...,Hs,Ws,3] or float32 [...,3,Hs,Ws] (got %s)" % photos.dtype)
    if clip is None:
        lo, hi = -math.inf, math.inf
    else:
        lo, hi = float(clip[0]), float(clip[1])
        if math.isnan(lo) or math.isnan(hi):
            raise ValueError("clip thresholds must not be NaN")
    P = int(np.prod(lead)) if lead else 1
    if P < 1 or Hs < 1 or Ws < 1:
        raise ValueError("photos must not be empty, got %s" % (tuple(photos.shape),))
    src = photos.contiguous()
    args = (fmt, P, int(Hs), int(Ws), Hd, Wd, int(samples), lo, hi)
    if any(isinstance(t, torch.Tensor) and t.requires_grad and torch.is_grad_enabled() for t in (matrices, lens)):
        return _Rectify.apply(_as_tensor(matrices), None if lens is None else _as_tensor(lens), src, lut, args, lead,
                              want_weights)
    return _launch_rectify(src, _device_matrices(matrices, lead, photos.device), lut, args, lead, want_weights,
                           None if lens is None else _device_lens(lens, lead, photos.device))


def _launch_rectify(src, mats, lut, args, lead, want_weights, lens=None):
    """the forward's one launch on checked arguments -> (values, weights or None): svbrdf_rectify_photos, or with the
    ``lens`` rows svbrdf_rectify_photos_lens"""
    fmt, P, Hs, Ws, Hd, Wd, k, lo, hi = args
    out = torch.empty(lead + (3, Hd, Wd), dtype=torch.float32, device=src.device)
    weights = torch.empty(lead + (Hd, Wd), dtype=torch.float32, device=src.device) if want_weights else None
    name, rows = ("svbrdf_rectify_photos", ()) if lens is None else ("svbrdf_rectify_photos_lens", (lens.data_ptr(),))
    _native._call(name, src.device, src.data_ptr(), fmt, P, Hs, Ws, mats.data_ptr(), *rows, Hd, Wd, k,
                  None if lut is None else lut.data_ptr(), lo, hi, out.data_ptr(),
                  None if weights is None else weights.data_ptr())
    return out, weights


class _Rectify(torch.autograd.Function):
    """``rectify`` for matrices and/or a lens that require grad (``lens`` may be None: the pinhole entries).  forward: the
    same launch.  backward: ONE launch of svbrdf_rectify_photos_grad_matrices, or with a lens of
    svbrdf_rectify_photos_lens_grad, on ``grad_output.contiguous()`` with the forward's saved arguments; each gradient comes
    back in the shape, dtype and device of its input (one matrix or one lens for all: the sum over the photos, added in
    float64), None for an input that did not ask.  Nothing towards the photos; the weights are non-differentiable; no
    double backward."""

    @staticmethod
    def forward(ctx, matrices, lens, src, lut, args, lead, want_weights):
        mats = _device_matrices(matrices.detach(), lead, src.device)
        rows = None if lens is None else _device_lens(lens.detach(), lead, src.device)
        out, weights = _launch_rectify(src, mats, lut, args, lead, want_weights, rows)
        ctx.save_for_backward(src, mats, rows, lut)
        ctx.args = args
        ctx.like = tuple(None if t is None else (t.shape, t.device, t.dtype) for t in (matrices, lens))
        ctx.shared = (matrices.dim() == (2 if matrices.shape[-2:] == (3, 3) else 1), lens is not None and lens.dim() == 1)
        if weights is not None:
            ctx.mark_non_differentiable(weights)
        return out, weights

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, _grad_weights=None):
        src, mats, rows, lut = ctx.saved_tensors
        fmt, P, Hs, Ws, Hd, Wd, k, lo, hi = ctx.args
        g = grad_out.to(torch.float32).contiguous().reshape(P, 3, Hd, Wd)
        if rows is None:
            grads = (_native.rectify_grad_matrices(src, fmt, P, Hs, Ws, mats, Hd, Wd, k, lut, lo, hi, g), None)
        else:
            grads = _native.rectify_lens_grad(src, fmt, P, Hs, Ws, mats, rows, Hd, Wd, k, lut, lo, hi, g)
        back = []
        for grad, like, shared, asked in zip(grads, ctx.like, ctx.shared, ctx.needs_input_grad):
            if not asked:
                back.append(None)
                continue
            shape, device, dtype = like
            if shared:
                grad = grad.to(torch.float64).sum(dim=0)
            back.append(grad.reshape(shape).to(device=device, dtype=dtype))
        return back[0], back[1], None, None, None, None, None


def to_perspective(renderings, camera_pos, sensor_size, t=1.0, samples=1):
    """The reference's ``OrthoToPerspectiveMapping(camera, sensor_size).apply(image, t)`` for device tensors: ``renderings``
    float32 ``[...,3,H,W]`` on the patch grid -> ``[...,3,sensor_size[1],sensor_size[0]]``, the patch as the camera at
    ``camera_pos`` sees it (one position ``[3]`` for all, or ``[...,3]``: one per image), zeros outside the patch like cv2's
    constant border.  ``t`` blends the mapping with the identity (the reference's animation parameter).  The float path of
    ``rectify``'s kernel with the inverse matrix, one launch; bilinear taps (cv2's default interpolation)."""
    if not isinstance(renderings, torch.Tensor) or renderings.dtype != torch.float32 or renderings.dim() < 3:
        raise TypeError("renderings must be a float32 [...,3,H,W] tensor")
    lead, size = tuple(renderings.shape[:-3]), tuple(renderings.shape[-2:])
    pos = np.asarray(camera_pos.detach().cpu() if isinstance(camera_pos, torch.Tensor) else camera_pos, np.float64)
    if pos.shape == (3,):
        mats = perspective_matrix(pos, sensor_size, size, t)
    elif pos.shape == lead + (3,):
        mats = np.stack([perspective_matrix(c, sensor_size, size, t) for c in pos.reshape(-1, 3)]).reshape(lead + (3, 3))
    else:
        raise ValueError("camera_pos must be [3] or %s, got %s" % (lead + (3,), pos.shape))
    return rectify(renderings, mats, (int(sensor_size[1]), int(sensor_size[0])), samples=samples, want_weights=False)[0]
