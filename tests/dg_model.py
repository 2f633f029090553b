"""A numpy model of the dynamic-GOP detector's early HME search (svtme_dg_detect, svtme_dg.hip).

A second restatement of early_hme_b64 and early_hme (pd_process.c:393-634), independent of
tests/golden/make_golden_dg.py, whose window() and metrics_of() made the fixtures, and of the
product. It searches the sixteenth planes of tests/pyramid_model.py. tests/test_dg.py pins it to
all ten fixtures (tests/golden/dg_cases.npz: the reference's planes and its sad_loop kernel).

DgModel's class attributes are the points where an implementation goes wrong quietly; a subclass
that changes one of them is a deliberately wrong variant (the discrimination test).
"""
import numpy as np

import pyramid_model as P

SB_DTYPE = np.dtype([("sad", "<u4"), ("mv_x", "<i2"), ("mv_y", "<i2")])  # svtme_dg_sb
METRIC_FIELDS = ("tot_dist", "tot_cplx", "tot_active", "sum_in_vectors", "mv_in_out_count", "perc_cplx",
                 "perc_active", "norm_dist")
CPLX_TH = 16 * 16 * 30


def c_div(a: int, b: int) -> int:
    """C integer division: toward zero."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def narrow(v: int, bits: int, signed: bool) -> int:
    v &= (1 << bits) - 1
    return v - (1 << bits) if signed and v >> (bits - 1) else v


class DgModel:
    pad = 16 - 1                  # the window may start `pad` samples into the margin
    width_mult8 = True            # widths of 8 and more lose their residue mod 8
    reduce_on_left_clamp = False  # the reference subtracts zero: the origin has moved by then
    first_wins = True             # a strict < keeps the first minimum
    y_major = True                # positions are visited row by row
    cplx_strict = True            # sad > 16 * 16 * 30
    trunc_div = True              # C division for mv_in_out_count

    def window(self, org: int, dim: int, sa: int, mult8: bool):
        """One axis of the clamp (pd_process.c:409-449): (sa_origin, sa, clamped low, clamped high).

        Python integers. The reference computes in int16_t; for pictures up to 16 384 wide
        dim <= 4096, 0 <= org < dim, 1 <= sa <= 128 and pad <= 16, so every intermediate value
        lies within +-(4096 + 128 + 16): the narrowing never changes a value and is not restated."""
        origin = -(sa >> 1)
        low = high = False
        if org + origin < -self.pad:
            moved = -self.pad - (org + origin)
            origin = -self.pad - org
            sa -= moved if self.reduce_on_left_clamp else -self.pad - (org + origin)
            low = True
        if org + origin > dim - 1:
            origin -= (org + origin) - (dim - 1)
            high = True
        if org + origin + sa > dim:
            sa = max(1, sa - ((org + origin + sa) - dim))
            high = True
        if mult8 and self.width_mult8 and sa >= 8:
            sa &= ~7
        return origin, sa, low, high

    def sb_windows(self, w: int, h: int, sa_w: int, sa_h: int):
        """Per 64x64 SB of the 8-aligned picture, raster order, at sixteenth resolution:
        (org_x, org_y, origin_x, origin_y, sw, sh, (left, right, top, bottom clamped))."""
        W, H = P.align8(w), P.align8(h)
        out = []
        for by in range((H + 63) // 64):
            for bx in range((W + 63) // 64):
                org_x, org_y = 16 * bx, 16 * by
                ox, sw, left, right = self.window(org_x, W // 4, (sa_w + 7) & ~7, True)
                oy, sh, top, bottom = self.window(org_y, H // 4, sa_h, False)
                out.append((org_x, org_y, ox, oy, sw, sh, (left, right, top, bottom)))
        return out

    @staticmethod
    def sads(six_c: np.ndarray, six_r: np.ndarray, win) -> np.ndarray:
        """[sh, sw]: the 16x16 SAD of the SB's block at every position of its window."""
        org_x, org_y, ox, oy, sw, sh = win[:6]
        pad = P.PAD_SIXTEENTH
        src = six_c[pad + org_y:pad + org_y + 16, pad + org_x:pad + org_x + 16].astype(np.int16)
        y0, x0 = pad + org_y + oy, pad + org_x + ox
        assert y0 >= 0 and x0 >= 0 and src.shape == (16, 16)
        area = six_r[y0:y0 + sh + 15, x0:x0 + sw + 15].astype(np.int16)
        assert area.shape == (sh + 15, sw + 15)
        view = np.lib.stride_tricks.sliding_window_view(area, (16, 16))
        return np.abs(view - src).sum(axis=(2, 3), dtype=np.int64)

    def pick(self, sad: np.ndarray):
        """(y, x) of the winning position."""
        s = sad if self.y_major else sad.T
        flat = s.ravel()
        k = int(np.argmin(flat)) if self.first_wins else flat.size - 1 - int(np.argmin(flat[::-1]))
        a, b = divmod(k, s.shape[1])
        return (a, b) if self.y_major else (b, a)

    def search(self, six_c: np.ndarray, six_r: np.ndarray, w: int, h: int, sa_w: int, sa_h: int,
               events: list = None) -> np.ndarray:
        """The per-SB results of one pair from the two sixteenth planes (margins included)."""
        wins = self.sb_windows(w, h, sa_w, sa_h)
        out = np.zeros(len(wins), SB_DTYPE)
        for k, win in enumerate(wins):
            sad = self.sads(six_c, six_r, win)
            y, x = self.pick(sad)
            out[k] = (int(sad[y, x]), (x + win[2]) * 4, (y + win[3]) * 4)
            if events is not None:
                events.append(sb_events(win, sad, y, x))
        return out

    def detect(self, cur: np.ndarray, ref: np.ndarray, sa_w: int, sa_h: int, events: list = None, pyramid=P.pyramid):
        """cur, ref: (h, w) luma planes (uint8, or uint16 searched on the MSB plane)
        -> (per-SB results, metrics in METRIC_FIELDS order)."""
        h, w = cur.shape
        sb = self.search(pyramid(cur)[2], pyramid(ref)[2], w, h, sa_w, sa_h, events)
        return sb, self.metrics(w, h, sb)

    def metrics(self, w: int, h: int, sb) -> list:
        """The frame metrics (pd_process.c:543-580, 630-633) in METRIC_FIELDS order."""
        wb, hb = (P.align8(w) + 63) // 64, (P.align8(h) + 63) // 64
        n = wb * hb
        assert len(sb) == n
        dist = cplx = active = vec = 0
        for k in range(n):
            sad, mx, my = int(sb["sad"][k]), int(sb["mv_x"][k]), int(sb["mv_y"][k])
            by, bx = divmod(k, wb)
            dist += sad
            cplx += (sad > CPLX_TH) if self.cplx_strict else (sad >= CPLX_TH)
            active += (mx != 0 or my != 0)
            # inwards or outwards; the middle row and the middle column count nothing
            if by != hb // 2:
                vec += np.sign(my) * (-1 if by < hb // 2 else 1)
            if bx != wb // 2:
                vec += np.sign(mx) * (-1 if bx < wb // 2 else 1)
        vec = int(vec)
        in_out = c_div(vec * 100, n) if self.trunc_div else (vec * 100) // n
        return [dist, cplx, active, vec, narrow(in_out, 16, True), narrow(c_div(cplx * 100, n), 8, False),
                narrow(c_div(active * 100, n), 8, False), dist // n]


def sb_events(win, sad: np.ndarray, y: int, x: int) -> dict:
    """What one SB's search exercises (the coverage test of tests/test_dg.py)."""
    org_x, org_y, ox, oy, sw, sh, clamped = win
    ys, xs = np.nonzero(sad == sad.min())  # raster order
    skew = False  # two minima 4 or more columns apart, the one in the earlier row in the later column
    for i in range(min(len(ys), 64)):
        later = ys > ys[i]
        if later.any() and (xs[i] - xs[later]).max() >= 4:
            skew = True
            break
    return {"sw": sw, "sh": sh, "x0_and_3": (org_x + ox) & 3, "clamped": clamped, "win_x": x, "win_y": y,
            "min_sad": int(sad.min()), "n_min": len(ys), "n_pos": sad.size,
            "min_row_span": int(ys.max() - ys.min()), "min_skew": skew,
            "mv_x": (x + ox) * 4, "mv_y": (y + oy) * 4}
