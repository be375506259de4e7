"""Float64 restatements for the face localizer's tests: the network with every BatchNorm folded into its convolution, block by block; the
letterbox of a frame into the 224 x 288 input; the map of the localizer's box to frame pixels; the re-acquisition rule of
ttk_track_reacquire.  Held to the reference's own LocalizerNet by tests/test_localizer_ref.py (tests/golden/localizer.npz); the GPU tests
compare the kernels against these."""
import numpy as np
import torch
import torch.nn.functional as F

IN_H, IN_W = 224, 288
# (in_ch, out_ch, kernel, stride, expansion) of convnet[2:14]
BLOCKS = ((8, 12, 3, 2, 2), (12, 12, 3, 1, 2), (12, 20, 3, 2, 4), (20, 20, 3, 1, 4), (20, 20, 3, 1, 4), (20, 32, 5, 2, 2),
          (32, 32, 5, 1, 2), (32, 32, 3, 1, 2), (32, 32, 3, 1, 2), (32, 56, 3, 2, 2), (56, 56, 3, 1, 2), (56, 56, 3, 1, 2))
TAPS = (1, 2, 8, 14)  # the convnet indices whose outputs the fixture stores
BN_EPS = 1e-5
MUL, ADD = 1.0 / 256.0, -0.5  # the whitening of the pose crops


def sample_grid(n, step=4):
    """Indices 0, step, 2 step, ... and n - 1: the rows / columns at which the fixture stores its two large intermediate tensors."""
    return np.unique(np.concatenate([np.arange(0, n, step), [n - 1]]))


def fold(sd, conv, bn):
    """(w', b') in float64: w' = w g / sqrt(var + eps), b' = beta - mean g / sqrt(var + eps)."""
    w = torch.as_tensor(np.asarray(sd[conv + ".weight"])).double()
    g = torch.as_tensor(np.asarray(sd[bn + ".weight"])).double() / torch.sqrt(torch.as_tensor(np.asarray(sd[bn + ".running_var"])).double() + BN_EPS)
    b = torch.as_tensor(np.asarray(sd[bn + ".bias"])).double() - torch.as_tensor(np.asarray(sd[bn + ".running_mean"])).double() * g
    return w * g[:, None, None, None], b


def block_forward(x, w1, b1, w2, b2, w3, b3, stride, residual):
    """One inverted-residual block on folded parameters (conv weights in torch's shapes), any dtype."""
    k = w2.shape[-1]
    e = F.relu(F.conv2d(x, w1, b1))
    d = F.relu(F.conv2d(e, w2, b2, stride=stride, padding=k // 2, groups=w2.shape[0]))
    y = F.conv2d(d, w3, b3)
    return y + x if residual else y


def block_unfused(x, p, stride, residual, eps=BN_EPS):
    """The same block as the module evaluates it - convolution, then eval-mode BatchNorm - in x's dtype.  p: dict with w1, w2, w3 and
    bn1, bn2, bn3 = (weight, bias, mean, var)."""
    k = p["w2"].shape[-1]
    t = lambda a: torch.as_tensor(a).to(x.dtype)
    bn = lambda v, q: F.batch_norm(v, t(q[2]), t(q[3]), t(q[0]), t(q[1]), False, 0.0, eps)
    e = F.relu(bn(F.conv2d(x, t(p["w1"])), p["bn1"]))
    d = F.relu(bn(F.conv2d(e, t(p["w2"]), stride=stride, padding=k // 2, groups=p["w2"].shape[0]), p["bn2"]))
    y = bn(F.conv2d(d, t(p["w3"])), p["bn3"])
    return y + x if residual else y


def fold_block(p, eps=BN_EPS):
    """block_unfused's parameters -> (w1, b1, w2, b2, w3, b3) folded in float64."""
    out = []
    for w, q in ((p["w1"], p["bn1"]), (p["w2"], p["bn2"]), (p["w3"], p["bn3"])):
        w, (g, beta, mean, var) = torch.as_tensor(w).double(), [torch.as_tensor(v).double() for v in q]
        s = g / torch.sqrt(var + eps)
        out += [w * s[:, None, None, None], beta - mean * s]
    return out


def pack(parts):
    """Folded float64 tensors -> one float32 vector in the order of include/ttk.h's parameter block."""
    return torch.cat([torch.as_tensor(v).double().reshape(-1) for v in parts]).to(torch.float32)


def folded_layers(sd):
    """The state dict -> (stem, dw, pw, [blocks], head): folded (w, b) pairs in float64."""
    stem = fold(sd, "convnet.0.0", "convnet.0.1")
    dw, pw = fold(sd, "convnet.1.0", "convnet.1.1"), fold(sd, "convnet.1.3", "convnet.1.4")
    blocks = []
    for i in range(len(BLOCKS)):
        pre = f"convnet.{i + 2}.layers."
        blocks.append(fold(sd, pre + "0", pre + "1") + fold(sd, pre + "3", pre + "4") + fold(sd, pre + "6", pre + "7"))
    head = (torch.as_tensor(np.asarray(sd["convnet.14.weight"])).double(), torch.as_tensor(np.asarray(sd["convnet.14.bias"])).double())
    return stem, dw, pw, blocks, head


def packed_parameters(sd, eps=1.0e-4):
    stem, dw, pw, blocks, head = folded_layers(sd)
    parts = list(stem) + list(dw) + list(pw)
    for b in blocks:
        parts += list(b)
    parts += list(head) + [torch.as_tensor(np.asarray(sd["boxstddev.half_size"])).double().reshape(1), torch.tensor([eps], dtype=torch.float64)]
    return pack(parts)


def position_code(n):
    return torch.linspace(-1.0, 1.0, n, dtype=torch.float32).double()  # float32 values, as the module builds them


def forward(sd, x, eps=1.0e-4):
    """x [B, 1, 224, 288] float64 -> (out [B, 5], attention [B, 7, 9], {tap: tensor}) in float64 on folded parameters."""
    stem, dw, pw, blocks, head = folded_layers(sd)
    x = torch.as_tensor(x).double()
    taps = {}
    z = F.relu(F.conv2d(x, stem[0], stem[1], stride=2, padding=1))
    z = F.conv2d(F.relu(F.conv2d(z, dw[0], dw[1], padding=1, groups=8)), pw[0], pw[1])
    taps[1] = z
    for i, ((cin, cout, k, stride, _), b) in enumerate(zip(BLOCKS, blocks)):
        z = block_forward(z, *b, stride=stride, residual=(cin == cout and stride == 1))
        taps[i + 2] = z
    z = F.conv2d(z, head[0], head[1])
    taps[14] = z
    logit = z[:, 0].mean(dim=[1, 2])
    att = torch.softmax(z[:, 1].reshape(z.shape[0], -1), dim=1).view(-1, 7, 9)
    half = float(np.asarray(sd["boxstddev.half_size"]))
    px, py = position_code(9)[None, None, :], position_code(7)[None, :, None]
    mean = torch.stack([half * (att * px).sum(dim=[1, 2]), half * (att * py).sum(dim=[1, 2])], dim=1)
    dx, dy = px - mean[:, 0, None, None], py - mean[:, 1, None, None]
    std = torch.sqrt(torch.stack([(att * dx * dx).sum(dim=[1, 2]), (att * dy * dy).sum(dim=[1, 2])], dim=1) + eps)
    out = torch.cat([logit[:, None], mean - std, mean + std], dim=1)
    return out, att, taps


# ---- letterbox ------------------------------------------------------------------------------------
def letterbox_geometry(Hs, Ws):
    s = min(IN_W / Ws, IN_H / Hs)
    return s, 0.5 * (IN_W - Ws * s), 0.5 * (IN_H - Hs * s)


def _overlap(n_out, n_src, s, o):
    """[n_out, n_src]: length of the overlap of source pixel j = [j, j + 1) with the pre-image [(i - o) / s, (i + 1 - o) / s) of output pixel i."""
    i, j = np.arange(n_out, dtype=np.float64)[:, None], np.arange(n_src, dtype=np.float64)[None, :]
    lo, hi = (i - o) / s, (i + 1 - o) / s
    return np.maximum(0.0, np.minimum(hi, j + 1) - np.maximum(lo, j))


def letterbox(frame, mul=None, add=None):
    """frame [Hs, Ws] -> (x [224, 288] float64, (s, ox, oy)): every input pixel is the exact area average of the frame over the pixel's
    pre-image, outside the frame counting as 0; with mul / add, times mul plus add."""
    f = np.asarray(frame, dtype=np.float64)
    s, ox, oy = letterbox_geometry(*f.shape)
    x = (_overlap(IN_H, f.shape[0], s, oy) @ f @ _overlap(IN_W, f.shape[1], s, ox).T) * (s * s)
    if mul is not None:
        x = x * mul + add
    return x, (s, ox, oy)


def box_to_frame(box, lb):
    """The localizer's box [..., 4] in [-1, 1] -> frame pixels, in float32 step by step as csrc/localizer_math.h rounds it:
    X = (x + 1) * 144, Y = (y + 1) * 112, then ((X - ox) / s, (Y - oy) / s).  lb [..., 3] = (s, ox, oy)."""
    box, lb = np.asarray(box, dtype=np.float32), np.asarray(lb, dtype=np.float32)
    half = np.array([IN_W / 2, IN_H / 2, IN_W / 2, IN_H / 2], dtype=np.float32)
    off = np.stack([lb[..., 1], lb[..., 2], lb[..., 1], lb[..., 2]], axis=-1)
    with np.errstate(all="ignore"):
        return (((box + np.float32(1)) * half - off) / lb[..., :1]).astype(np.float32)


def sigmoid32(v):
    with np.errstate(all="ignore"):
        return (np.float32(1) / (np.float32(1) + np.exp(-np.asarray(v, dtype=np.float32)))).astype(np.float32)


def candidate(roi, factor, Ws, Hs):
    """(clamped box, valid): the tracker's box rule in float32 (include/ttk.h, ttk_track_update)."""
    r = np.asarray(roi, dtype=np.float32)
    with np.errstate(all="ignore"):
        c = np.array([np.fmax(np.float32(0), r[0]), np.fmax(np.float32(0), r[1]), np.fmin(r[2], np.float32(Ws)), np.fmin(r[3], np.float32(Hs))], dtype=np.float32)
        w, h = np.float32(c[2] - c[0]), np.float32(c[3] - c[1])
        valid = bool(np.all(np.isfinite(r)) and w > 0 and h > 0 and np.float32(np.fmax(w, h) * np.float32(factor)) >= 2)
    return c, valid


def reacquire_rule(loc_out, lb, lost_row, lane_seq, lane_factor, roi_state, lost_run, Hs, Ws, reacquire_after, face_threshold):
    """One frame of ttk_track_reacquire.  Returns (roi_state, lost_run, reacquired [L], hasface [S], loc_roi [S, 4]); the inputs stay."""
    loc_out, lb = np.asarray(loc_out, dtype=np.float32), np.asarray(lb, dtype=np.float32)
    roi_state, lost_run = np.array(roi_state, dtype=np.float32), np.array(lost_run, dtype=np.int32)
    hasface, loc_roi = sigmoid32(loc_out[:, 0]), box_to_frame(loc_out[:, 1:], lb)
    reacquired = np.zeros(len(lane_seq), dtype=bool)
    for l, q in enumerate(lane_seq):
        run = lost_run[l] + 1 if lost_row[l] else 0
        take = False
        if run >= reacquire_after:
            c, valid = candidate(loc_roi[q], lane_factor[l], Ws, Hs)
            take = valid and bool(hasface[q] > np.float32(face_threshold))
            if take:
                roi_state[l] = c
        lost_run[l] = 0 if take else run
        reacquired[l] = take
    return roi_state, lost_run, reacquired, hasface, loc_roi
