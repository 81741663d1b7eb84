"""The numpy binary32 restatement of include/pt_render.h's temporal reprojection (PtTemporal, pt_temporal_push): what
tests/test_gpu_temporal.py holds the kernel to bit for bit, and what tests/test_temporal_cpu.py checks the header's promises on.

Every array is float32, every operation is rounded once (a product is rounded before it enters a sum), the order of operations is the
header's.  Cameras are anything with PtCamera's fields (abi.PtCamera, or an object with origin, lower_left_corner, horizontal, vertical,
w as sequences of 3)."""
import numpy as np

F = np.float32
DEFAULTS = dict(alpha=0.1, tol_depth=0.1, tol_normal=0.5)
N_MAX = F(65536.0)


def cam_vectors(cam):
    return {k: np.array([float(x) for x in getattr(cam, k)], F) for k in ("origin", "lower_left_corner", "horizontal", "vertical", "w")}


def dot3(ax, ay, az, b):
    """(a.x b.x + a.y b.y) + a.z b.z with every product and sum rounded."""
    return ((ax * b[0] + ay * b[1]) + az * b[2]).astype(F) if isinstance(ax, np.ndarray) else F(F(F(ax * b[0]) + F(ay * b[1])) + F(az * b[2]))


def host_constants(cam):
    """(fo, hh, vv) of a camera as pt_temporal_push takes them for the PREVIOUS camera; None for a degenerate one."""
    c = cam_vectors(cam)
    g = (c["lower_left_corner"] - c["origin"]).astype(F)
    with np.errstate(all="ignore"):
        fo = F(-dot3(g[0], g[1], g[2], c["w"]))
        hh = dot3(*c["horizontal"], c["horizontal"])
        vv = dot3(*c["vertical"], c["vertical"])
    if not all(np.isfinite(v) and v > 0 for v in (fo, hh, vv)):
        return None
    return fo, hh, vv


class Temporal:
    """The history of one image sequence: per pixel c, m2 [H][W][3], N, z [H][W], n [H][W][3], k [H][W] int32; the last camera."""

    def __init__(self, width, height):
        self.width, self.height = int(width), int(height)
        self.reset()

    def reset(self):
        self.frames = 0
        self.cam = None
        h, w = self.height, self.width
        self.c, self.m2, self.n = (np.zeros((h, w, 3), F) for _ in range(3))
        self.N, self.z = np.zeros((h, w), F), np.zeros((h, w), F)
        self.k = np.zeros((h, w), np.int32)

    def push(self, cam, color, depth, normal=None, id=None, variance_in=None, alpha=0.1, tol_depth=0.1, tol_normal=0.5):
        """One pt_temporal_push -> (out_color, out_variance, out_history)."""
        if host_constants(cam) is None:
            raise ValueError("degenerate camera")
        W, H = self.width, self.height
        C = np.ascontiguousarray(color, F).reshape(H, W, 3)
        z = np.ascontiguousarray(depth, F).reshape(H, W)
        nrm = None if normal is None else np.ascontiguousarray(normal, F).reshape(H, W, 3)
        kid = None if id is None else np.ascontiguousarray(id, np.int32).reshape(H, W)
        alpha, tol_depth, tol_normal = F(alpha), F(tol_depth), F(tol_normal)
        one = F(1.0)
        with np.errstate(all="ignore"):
            finite = (np.abs(C) < np.inf).all(axis=2)
            CC = (C * C).astype(F)
            have = np.zeros((H, W), bool)  # pixels that take the history
            hcn, hmn, Nn = np.zeros((H, W, 3), F), np.zeros((H, W, 3), F), np.ones((H, W), F)
            if self.frames > 0:
                cur, prev = cam_vectors(cam), cam_vectors(self.cam)
                prev_h, prev_v = cam_vectors(self.cam)["horizontal"], cam_vectors(self.cam)["vertical"]
                fo, hh, vv = host_constants(self.cam)
                xs = np.arange(W, dtype=F)[None, :].repeat(H, 0)
                ys = np.arange(H, dtype=F)[:, None].repeat(W, 1)
                sc = ((xs + F(0.5)) / F(W)).astype(F)
                tc = ((ys + F(0.5)) / F(H)).astype(F)
                dirv = [(((cur["lower_left_corner"][a] + sc * cur["horizontal"][a]) + tc * cur["vertical"][a]) - cur["origin"][a]).astype(F)
                        for a in range(3)]
                hit = z > 0
                d = [np.where(hit, ((cur["origin"][a] + z * dirv[a]) - prev["origin"][a]).astype(F), dirv[a]) for a in range(3)]
                cp = (-dot3(d[0], d[1], d[2], prev["w"])).astype(F)
                r = (fo / cp).astype(F)
                te = (cp / fo).astype(F)
                s1 = ((dot3(d[0], d[1], d[2], prev_h) * r) / hh + F(0.5)).astype(F)
                t1 = ((dot3(d[0], d[1], d[2], prev_v) * r) / vv + F(0.5)).astype(F)
                fx = (s1 * F(W) - F(0.5)).astype(F)
                fy = (t1 * F(H) - F(0.5)).astype(F)
                usable = (cp > 0) & (fx >= -1) & (fx < F(W)) & (fy >= -1) & (fy < F(H))
                fx0 = np.where(usable, np.floor(fx), F(0)).astype(F)
                fy0 = np.where(usable, np.floor(fy), F(0)).astype(F)
                ax, ay = (fx - fx0).astype(F), (fy - fy0).astype(F)
                x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
                hc, hm = np.zeros((H, W, 3), F), np.zeros((H, W, 3), F)
                hN, bs = np.zeros((H, W), F), np.zeros((H, W), F)
                tn2 = F(tol_normal * tol_normal)
                tol_te = (tol_depth * te).astype(F)
                for j in (0, 1):
                    for i in (0, 1):
                        qx, qy = x0 + i, y0 + j
                        inside = usable & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                        qxc, qyc = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                        b = ((ax if i else (one - ax).astype(F)) * (ay if j else (one - ay).astype(F))).astype(F)
                        Nq, zq = self.N[qyc, qxc], self.z[qyc, qxc]
                        ok = inside & (Nq >= 1)
                        ok &= np.where(hit, (zq > 0) & (np.abs((zq - te).astype(F)) <= tol_te), ~(zq > 0))
                        if kid is not None:
                            ok &= self.k[qyc, qxc] == kid
                        if nrm is not None:
                            dn = (nrm - self.n[qyc, qxc]).astype(F)
                            ok &= ((dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]).astype(F) <= tn2
                        hc = np.where(ok[..., None], (hc + b[..., None] * self.c[qyc, qxc]).astype(F), hc)
                        hm = np.where(ok[..., None], (hm + b[..., None] * self.m2[qyc, qxc]).astype(F), hm)
                        hN = np.where(ok, (hN + b * Nq).astype(F), hN)
                        bs = np.where(ok, (bs + b).astype(F), bs)
                have = usable & (bs > F(0.01))
                safe = np.where(have, bs, one)
                hcn = (hc / safe[..., None]).astype(F)
                hmn = (hm / safe[..., None]).astype(F)
                Nn = np.where(have, np.fmin((hN / safe + one).astype(F), N_MAX), one).astype(F)
            a_p = np.where(have, np.fmax((one / Nn).astype(F), alpha), one).astype(F)
            c = np.where(have[..., None], (hcn + a_p[..., None] * (C - hcn).astype(F)).astype(F), C)
            m2 = np.where(have[..., None], (hmn + a_p[..., None] * (CC - hmn).astype(F)).astype(F), CC)
            var = (np.fmax((m2 - (c * c).astype(F)).astype(F), F(0)) * a_p[..., None]).astype(F)
            young = np.full((H, W, 3), np.inf, F) if variance_in is None else np.ascontiguousarray(variance_in, F).reshape(H, W, 3)
            out_var = np.where((Nn >= 4)[..., None], var, young)
            out_color, out_hist = c.copy(), Nn.copy()
            # a pixel whose colour is not finite: it stays where it is and never enters a history
            out_color[~finite] = C[~finite]
            out_var[~finite] = np.inf
            out_hist[~finite] = 0
            c[~finite] = 0
            m2[~finite] = 0
            Nn = np.where(finite, Nn, F(0)).astype(F)
        self.c, self.m2, self.N, self.z = c, m2, Nn, z.copy()
        self.n = np.zeros((H, W, 3), F) if nrm is None else nrm.copy()
        self.k = np.zeros((H, W), np.int32) if kid is None else kid.copy()
        self.cam = _copy_cam(cam)
        self.frames += 1
        return out_color.astype(F), out_var.astype(F), out_hist.astype(F)


class _Cam:
    pass


def _copy_cam(cam):
    c = _Cam()
    for k, v in cam_vectors(cam).items():
        setattr(c, k, v.copy())
    return c
