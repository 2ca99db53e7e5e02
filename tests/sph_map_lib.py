"""The two SPH mappings of include/cmi_gpu.h ("SPH mappings") as a numpy brute
force over ALL (particle, cell midpoint) pairs: both kernel forms, the
minimum image of a periodic box, and the derived tolerance of every output.
Also the test cases the CPU and GPU tests share.

Nothing here knows of tiles, lists or classes: a pair contributes when its
separation is inside the kernel's support, and that is all."""
import numpy as np

KC1, KC2, KC5 = 2.546479089470, 15.278874536822, 5.092958178941
EPS = 2. ** -53


def midpoints(anchor, sides, ncell):
    """(ncells, 3), z fastest; the host grid's own operations:
    (anchor + side * i) + 0.5 * side with side = sides / ncell."""
    axes = []
    for a in range(3):
        side = float(sides[a]) / int(ncell[a])
        axes.append((float(anchor[a]) + side * np.arange(int(ncell[a]))) +
                    0.5 * side)
    X, Y, Z = np.meshgrid(*axes, indexing="ij")
    return np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)


def reach_of(form, h):
    return 2. * h if form == 1 else 1. * h


def kernel(form, r, h):
    """form 0: cubic_spline_kernel of SPHArrayInterface.hpp, support h;
    form 1: SphKernelDensityFunction::kernel (Price 2007), support 2 h. The
    host's sequence of operations."""
    u = r / h
    h3 = h * h * h
    if form == 0:
        inner = (KC1 + KC2 * (u - 1.) * u * u) / h3
        outer = KC5 * (1. - u) * (1. - u) * (1. - u) / h3
        return np.where(u < 1., np.where(u < 0.5, inner, outer), 0.)
    u2 = u * u
    inner = (1. - 1.5 * u2 + 0.75 * u2 * u) / (np.pi * h3)
    c = 2. - u
    outer = 0.25 * (c * c) * c / (np.pi * h3)
    return np.where(u < 1., inner, np.where(u < 2., outer, 0.))


def central_value(form, h):
    """W(0, h)"""
    return (KC1 if form == 0 else 1. / np.pi) / (h * h * h)


def separation(c, p, box_sides):
    """per axis, the minimum image applied once as Box::periodic_distance"""
    d = c - p
    if box_sides is not None:
        L = np.asarray(box_sides, dtype=np.float64)
        d = np.where(2. * d < -L, d + L, d)
        d = np.where(2. * d >= L, d - L, d)
    return d


class Pairs:
    """Every contributing pair of a case and a kernel form: particle i, cell
    c, weight W(|c - p_i|, h_i)."""

    def __init__(self, positions, h, form, grid, periodic_box=None,
                 chunk=256):
        anchor, sides, ncell = grid
        pos = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
        h = np.asarray(h, dtype=np.float64)
        mid = midpoints(anchor, sides, ncell)
        box = None if periodic_box is None else np.asarray(
            periodic_box, dtype=np.float64).reshape(6)[3:]
        self.n, self.ncells, self.form, self.h = len(h), len(mid), form, h
        ii, cc, ww = [], [], []
        for first in range(0, len(h), chunk):
            p = pos[first:first + chunk]
            hh = h[first:first + chunk]
            d = separation(mid[None, :, :], p[:, None, :], box)
            r = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) +
                        d[..., 2] * d[..., 2])
            i, c = np.nonzero(r < reach_of(form, hh)[:, None])
            w = kernel(form, r[i, c], hh[i])
            keep = w > 0.
            ii.append(i[keep] + first)
            cc.append(c[keep])
            ww.append(w[keep])
        self.i = np.concatenate(ii) if ii else np.zeros(0, dtype=np.int64)
        self.c = np.concatenate(cc) if cc else np.zeros(0, dtype=np.int64)
        self.w = np.concatenate(ww) if ww else np.zeros(0)
        self.w0 = central_value(form, h)[self.i]

    def to_cells(self, amplitudes):
        """out[K][ncells] and the bound tol[K][ncells] =
        (8 + n) 2^-53 sum |a_i| W(0, h_i) over the n contributing pairs"""
        amp = np.asarray(amplitudes, dtype=np.float64).reshape(-1, self.n)
        count = np.bincount(self.c, minlength=self.ncells)
        out = np.stack([np.bincount(self.c, weights=a[self.i] * self.w,
                                    minlength=self.ncells) for a in amp])
        tol = np.stack([(8 + count) * EPS *
                        np.bincount(self.c,
                                    weights=np.abs(a[self.i]) * self.w0,
                                    minlength=self.ncells) for a in amp])
        return out, tol

    def to_particles(self, values):
        """out[n] and tol[n], the same bound with |g_c| W(0, h_i)"""
        g = np.asarray(values, dtype=np.float64).reshape(self.ncells)
        count = np.bincount(self.i, minlength=self.n)
        out = np.bincount(self.i, weights=self.w * g[self.c],
                          minlength=self.n)
        tol = (8 + count) * EPS * np.bincount(
            self.i, weights=np.abs(g[self.c]) * self.w0, minlength=self.n)
        return out, tol


def assert_within(got, expect, tol, what):
    """|got - expect| <= tol everywhere; outputs without a contributing pair
    (tol = 0 and expect = 0) exactly 0"""
    got = np.asarray(got).reshape(np.shape(expect))
    err = np.abs(got - expect)
    worst = np.max(err / np.where(tol > 0., tol, 1.)) if err.size else 0.
    print("%s: worst error / bound = %.3g over %d outputs, %d with no pair" %
          (what, worst, err.size, int(np.sum(tol == 0.))))
    empty = tol == 0.
    assert np.all(got[empty] == 0.), what + ": an output no pair reaches is " \
        "not exactly 0"
    bad = err > tol
    assert not bad.any(), "%s: %d outputs beyond the bound, worst %.3g x" % (
        what, int(bad.sum()), worst)


# ------------------------------------------------------------------ cases --

GRID_A = ((-1.5, 2., 10.), (6., 4., 3.2), (12, 10, 8))  # sides of 0.5, 0.4, 0.4


def case_a(periodic=False):
    """Geometry: a 12 x 10 x 8 grid in a box with three different sides, about
    600 particles with h from 0.3 to 4 cell sides (some cover no midpoint,
    some span several tiles), some outside the box whose kernel reaches in,
    some far outside, one exactly on a cell midpoint; a corner region that no
    particle covers. periodic: case B, the periodic box is the grid and the
    kernels cross all six faces and the corners."""
    anchor, sides, ncell = (np.array(GRID_A[0]), np.array(GRID_A[1]),
                            GRID_A[2])
    cell = sides / np.array(ncell)
    rng = np.random.default_rng(11)
    inside = anchor + rng.uniform(0., 1., (500, 3)) * sides
    h_in = np.exp(rng.uniform(np.log(0.3), np.log(4.), len(inside))) * cell[1]
    # just outside each face, reaching in
    near = []
    for a in range(3):
        for sign in (-1., 1.):
            p = anchor + rng.uniform(0.4, 1., (10, 3)) * sides
            p[:, a] = (anchor[a] + (sides[a] if sign > 0 else 0.) +
                       sign * rng.uniform(0.05, 0.6, 10) * cell[a])
            near.append(p)
    near = np.concatenate(near)
    h_near = rng.uniform(1.5, 3., len(near)) * cell[0]
    far = anchor + sides * rng.uniform(3., 5., (20, 3)) * rng.choice(
        [-1., 1.], (20, 3))
    h_far = rng.uniform(0.3, 4., 20) * cell[1]
    # corners and faces: particles hugging them (they matter when periodic)
    corner = anchor + sides * rng.integers(0, 2, (16, 3)) + \
        rng.uniform(-0.2, 0.2, (16, 3)) * cell
    h_corner = rng.uniform(1., 2.5, len(corner)) * cell[1]
    on_mid = midpoints(anchor, sides, ncell)[[5 * 80 + 6 * 8 + 3]]
    pos = np.concatenate([inside, near, far, corner, on_mid])
    h = np.concatenate([h_in, h_near, h_far, h_corner, [1.7 * cell[1]]])
    if periodic:
        # 2 reach < smallest side for both forms: 2 * 2h < 3.2
        h = np.minimum(h, 0.24 * sides.min())
    else:
        # the cell in the low corner stays empty: whoever could reach its
        # midpoint with either form goes to the opposite side of the grid
        first = midpoints(anchor, sides, ncell)[0]
        reaches = np.linalg.norm(pos - first, axis=1) < 2.1 * h
        pos[reaches] = 2. * anchor + sides - pos[reaches]
    amp = rng.uniform(0.5, 2., (3, len(h)))
    g = rng.uniform(0.1, 1., int(np.prod(ncell)))
    box = np.concatenate([anchor, sides]) if periodic else None
    return dict(positions=np.ascontiguousarray(pos), h=h, amplitudes=amp,
                cell_values=g, grid=(anchor, sides, ncell), periodic_box=box)


def case_c():
    """Lists and classes: a 32 x 32 x 24 grid and 8000 particles, 3000 of
    them in a clump inside one cell (tile lists longer than the staging
    chunk), h on both sides of the lane/wave threshold of 64 candidates."""
    anchor, sides, ncell = np.zeros(3), np.array([1., 1., 0.75]), (32, 32, 24)
    cell = 1. / 32
    rng = np.random.default_rng(12)
    field = anchor + rng.uniform(0., 1., (5000, 3)) * sides
    # 2 h / cell from 0.8 (no or one candidate) to 7 (343 candidates)
    h_field = rng.uniform(0.4, 3.5, 5000) * cell
    clump = (np.array([13, 7, 9]) + rng.uniform(0.05, 0.95, (3000, 3))) * cell
    h_clump = rng.uniform(0.9, 2.6, 3000) * cell
    pos = np.concatenate([field, clump])
    h = np.concatenate([h_field, h_clump])
    amp = rng.uniform(0.5, 2., (3, len(h)))
    g = rng.uniform(0.1, 1., int(np.prod(ncell)))
    return dict(positions=np.ascontiguousarray(pos), h=h, amplitudes=amp,
                cell_values=g, grid=(anchor, sides, ncell), periodic_box=None)
