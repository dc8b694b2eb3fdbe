#!/usr/bin/env python3
"""Ground-plane positions of the reference's own evaluation sequence, as NUMBERS only -> tests/golden/terrace_geometry.npz.

Reads, as data, the annotation files and the per-camera homographies shipped with the reference (datasets/EPFL-Terrace/terrace1-c{0..3}:
gt/gt.txt and Homography.txt) and projects every annotated box onto the ground plane by the steps the reference's
loader documents (libs/datasets.py:93-113): rows with lost == 0; xmin + 1; the foot point (xmin + round(width / 2), ymax) with
width = xmax - xmin; the image-to-world homography applied to (x, y, 1) and divided by its third component.  A frame is valid when its
detections come from more than one camera and at least one identity is seen twice (libs/datasets.py:226-232), as in
make_terrace_topology.py, whose detection order (camera by camera, file order inside a camera) this file keeps.

Per valid frame the file stores the frame number and, per detection, camera id, person id and xw, yw as float64.  No image, no annotation
text and no code of the reference is stored.  Every valid frame is kept if the file then stays below the largest golden file of the
repository and below the 1 MiB limit of a committed file; otherwise the frames whose number is a multiple of 5 (what is committed: all
4816 valid frames take 1.14 MiB).

Prints the numbers tests/test_graph_radius_oracle.py records (the recall table of the radius gate on the stored frames).

Run in the build container only:   python tests/golden/make_terrace_geometry.py
"""
import os
import sys

import numpy as np

REF = "/root/reference/datasets/EPFL-Terrace"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "terrace_geometry.npz")
sys.path.insert(0, os.path.dirname(HERE))


def detections():
    """float64 rows (frame, cam, id, xw, yw) in the data set's concatenation order: camera by camera, file order inside a camera."""
    rows = []
    for c in sorted(d for d in os.listdir(REF) if os.path.isdir(os.path.join(REF, d))):
        a = np.loadtxt(os.path.join(REF, c, "gt", "gt.txt"), usecols=(0, 1, 2, 3, 4, 5, 6), dtype=np.float64)   # id xmin ymin xmax ymax frame lost
        a = a[a[:, 6] == 0]
        h = np.loadtxt(os.path.join(REF, c, "Homography.txt"), dtype=np.float64).reshape(3, 3)
        xmin = a[:, 1] + 1
        foot_x, foot_y = xmin + np.round((a[:, 3] - xmin) / 2), a[:, 4]
        p = h @ np.stack([foot_x, foot_y, np.ones_like(foot_x)])
        rows.append(np.stack([a[:, 5], np.full(len(a), float(c[-1:])), a[:, 0], p[0] / p[2], p[1] / p[2]], axis=1))
    return np.concatenate(rows)


def select(det, every):
    det = det[np.argsort(det[:, 0], kind="stable")]   # stable: keeps the camera-by-camera order inside a frame
    frames, starts = np.unique(det[:, 0], return_index=True)
    ends = np.concatenate([starts[1:], [len(det)]])
    keep, ptr = [], [0]
    valid = []
    for f, s, e in zip(frames.astype(np.int64), starts, ends):
        d = det[s:e]
        if f % every == 0 and len(np.unique(d[:, 1])) > 1 and np.bincount(d[:, 2].astype(np.int64)).max() > 1:
            valid.append(f)
            keep.append(d)
            ptr.append(ptr[-1] + len(d))
    d = np.concatenate(keep)
    return dict(frame=np.asarray(valid, np.int32), node_ptr=np.asarray(ptr, np.int32), cam=d[:, 1].astype(np.uint8), person=d[:, 2].astype(np.uint8),
                xw=d[:, 3].copy(), yw=d[:, 4].copy())


def main():
    det = detections()
    limit = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if os.path.join(HERE, f) != OUT)
    for every in (1, 5):
        z = select(det, every)
        np.savez_compressed(OUT, **z)
        size = os.path.getsize(OUT)
        print(f"every {every}: {len(z['frame'])} valid frames, {size} bytes (largest golden file: {limit})")
        if size < limit and size < (1 << 20):
            break
    import graph_radius_oracle as gro
    a = gro.terrace()
    sizes = a["graph_sizes"]
    table, e, pos, far = gro.recall_table(a, (40, 60, 80, 100, 150))
    print(f"{len(sizes)} frames; detections/frame mean {sizes.mean():.1f} max {sizes.max()}; {e} directed cross-camera edges, {pos} same-identity; "
          f"largest same-identity distance {far:.2f}")
    for r, kept, rec in table:
        print(f"radius {r}: kept {kept} ({kept / e:.4f}) same-identity kept {rec} ({rec / pos:.4f})")


if __name__ == "__main__":
    main()
