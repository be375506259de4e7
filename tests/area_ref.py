"""float64 restatement of the area-filtered crop (include/ttk.h, ttk_area_crop), written from its definition:

  Rx = max(N, round(N / |row 0 of tr|)), Ry likewise; kx = Rx / N, ky = Ry / N
  I[p][q] = bilinear(src, tr^-1((q + .5) / kx, (p + .5) / ky) - .5), zeros outside the source, p < Ry, q < Rx
  out[i][j] = sum_p sum_q wy[i][p] wx[j][q] I[p][q],  wx[j][q] = |[q, q + 1) n [j kx, (j + 1) kx)| / kx

`tr` is taken as the float32 values the kernel reads; everything after that is float64.  TEST INFRASTRUCTURE."""
import numpy as np


def extent(row, N):
    return max(N, int(np.rint(N / np.hypot(row[0], row[1]))))


def weights(N, R):
    """[N, R]: the share of intermediate cell q in output cell j; every row sums to 1."""
    k = R / N
    j, q = np.arange(N, dtype=np.float64)[:, None], np.arange(R, dtype=np.float64)[None, :]
    return np.clip(np.minimum(q + 1, (j + 1) * k) - np.maximum(q, j * k), 0.0, None) / k


def bilinear(img, u, v):
    """img (H, W) at the continuous pixel indices (u = column, v = row), zero padding."""
    H, W = img.shape
    x0, y0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    ax, ay = u - x0, v - y0

    def at(y, x):
        ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        return np.where(ok, img[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)], 0.0)

    return (at(y0, x0) * (1 - ax) + at(y0, x0 + 1) * ax) * (1 - ay) + (at(y0 + 1, x0) * (1 - ax) + at(y0 + 1, x0 + 1) * ax) * ay


def intermediate(img, tr, N):
    m = np.asarray(tr, np.float32).astype(np.float64)
    Rx, Ry = extent(m[0], N), extent(m[1], N)
    X, Y = np.meshgrid((np.arange(Rx) + 0.5) * N / Rx, (np.arange(Ry) + 0.5) * N / Ry)
    src = np.stack([X - m[0, 2], Y - m[1, 2]], -1) @ np.linalg.inv(m[:, :2]).T
    return bilinear(np.asarray(img, np.float64), src[..., 0] - 0.5, src[..., 1] - 0.5)


def area_crop(img, tr, N):
    """img (H, W), tr (2, 3) -> (N, N) float64 in the units of img (no mul / add)."""
    I = intermediate(img, tr, N)
    return weights(N, I.shape[0]) @ I @ weights(N, I.shape[1]).T


def area_crop_batch(imgs, trs, N):
    return np.stack([area_crop(im, t, N) for im, t in zip(imgs, trs)])


def roi_transform(view, N, angle=0.0):
    """The crop transform of an integer view ROI (x0, y0, x1, y1) as the loader composes it: rotation about the crop centre after the remap."""
    x0, y0, x1, y1 = [float(v) for v in view]
    sx, sy, c, s, h = N / (x1 - x0), N / (y1 - y0), np.cos(angle), np.sin(angle), 0.5 * N
    rot = np.array([[c, -s, h - (c * h - s * h)], [s, c, h - (s * h + c * h)], [0, 0, 1]])
    return (rot @ np.array([[sx, 0, -x0 * sx], [0, sy, -y0 * sy], [0, 0, 1]]))[:2].astype(np.float32)
