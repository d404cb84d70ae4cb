"""Image footprint of one gather instruction of k_integrate, by the sub-box of the block that the 64 lanes of a wave cover (CPU only, numpy).

A gather instruction reads one 8-byte record {depth, rgba} per lane from the row-major packed image of a frame.  For random views of a block of
5 mm voxels at 0.6 .. 3.5 m (half of them yaw-only with up to 0.3 rad of pitch, half random rotations; 640 x 480, f = 515) this counts, per
instruction, the distinct 128-byte lines, 64-byte sectors and pixels its 64 addresses fall into.  Pixels off the image are dropped, as the
buffer descriptor drops them.  Usage: python tools/kc_lane_footprint.py [views] [seed] > profiles/kc_lanes_footprint.txt
"""
import sys

import numpy as np

W, H, F, CX, CY, RES = 640, 480, 515.0, 319.5, 239.5, 0.005
COVERS = [(8, 8, 1), (8, 4, 2), (4, 8, 2), (8, 2, 4), (4, 4, 4), (2, 8, 4), (8, 1, 8)]


def rotations(n, rng):
    """n / 2 yaw-only views with a pitch of +-0.3 rad, n / 2 uniformly random rotations (QR of a Gaussian matrix, det +1)."""
    out = []
    for i in range(n):
        if i % 2 == 0:
            a, b = rng.uniform(-np.pi, np.pi), rng.uniform(-0.3, 0.3)
            ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
            rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
            out.append(rx @ ry)
        else:
            q, r = np.linalg.qr(rng.normal(size=(3, 3)))
            q = q * np.sign(np.diag(r))
            if np.linalg.det(q) < 0:
                q[:, 0] = -q[:, 0]
            out.append(q)
    return np.array(out)


def views(n, seed):
    """n views of a block: rotations, and the block's centre in camera coordinates somewhere in the image at a depth of 0.6 .. 3.5 m"""
    rng = np.random.default_rng(seed)
    R = rotations(n, rng)
    zc = rng.uniform(0.6, 3.5, n)
    centre = np.stack([(rng.uniform(0, W, n) - CX) / F * zc, (rng.uniform(0, H, n) - CY) / F * zc, zc], axis=1)
    return R, centre


def footprint(cover, R, centre):
    """Per view, for one gather instruction of a wave whose lanes cover `cover` = (bx, by, bz) voxels (every sub-box position in turn): arrays of the
    distinct 128-byte lines, 64-byte sectors and pixels among its on-image addresses."""
    bx, by, bz = cover
    nx, ny, nz = 8 // bx, 8 // by, 8 // bz
    g = (np.arange(8) - 3.5) * RES
    lines, sectors, pixels = [], [], []
    for k in range(len(R)):
        b = k % (nx * ny * nz)
        x0, y0, z0 = (b % nx) * bx, (b // nx % ny) * by, (b // (nx * ny)) * bz
        X, Y, Z = np.meshgrid(g[x0:x0 + bx], g[y0:y0 + by], g[z0:z0 + bz], indexing="ij")
        p = np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1) @ R[k].T + centre[k]
        u = np.rint(p[:, 0] / p[:, 2] * F + CX).astype(np.int64)
        v = np.rint(p[:, 1] / p[:, 2] * F + CY).astype(np.int64)
        ok = (u >= 0) & (u < W) & (v >= 0) & (v < H) & (p[:, 2] > 0)
        byte = (v[ok] * W + u[ok]) * 8
        if byte.size == 0:
            continue
        lines.append(np.unique(byte // 128).size)
        sectors.append(np.unique(byte // 64).size)
        pixels.append(np.unique(byte).size)
    return np.array(lines), np.array(sectors), np.array(pixels)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
    R, centre = views(n, int(sys.argv[2]) if len(sys.argv) > 2 else 1)
    print("views %d, %d x %d, f = %g, voxel %g m, 8-byte records" % (n, W, H, F, RES))
    print("%-9s %28s %18s %16s" % ("cover", "128-B lines mean (p50, p90)", "64-B sectors mean", "pixels mean"))
    for bx, by, bz in COVERS:
        lines, sectors, pixels = footprint((bx, by, bz), R, centre)
        print("%dx%dx%-5d %12.1f (%2.0f, %2.0f) %22.1f %18.1f" % (bx, by, bz, lines.mean(), np.percentile(lines, 50), np.percentile(lines, 90), np.mean(sectors), np.mean(pixels)))


if __name__ == "__main__":
    main()
