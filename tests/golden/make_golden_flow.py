"""Writes the optical-flow fixtures: the reference's two 752 x 480 test images as uint8 arrays (flow_image_1.npz, flow_image_2.npz) and
the keypoints of image 1 (flow_keypoints.npz).

    python tests/golden/make_golden_flow.py DIR        # DIR holds 1.png and 2.png (the reference's data/01-optical-flow)

The keypoints stand in for the reference's GFTTDetector: the Shi-Tomasi response (the smaller eigenvalue of the 5 x 5 box sum of the
central-difference gradient products) in numpy, at least MARGIN pixels from the image edge (a half patch of 4 at the top of a
4-level pyramid), the best pixel of every 32 x 32 cell, kept if its response is above 1 % of the largest.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CELL, QUALITY, MARGIN, BOX = 32, 0.01, 32, 5


def read_gray(path):
    from PIL import Image
    im = Image.open(path)
    assert im.mode == "L", im.mode
    return np.asarray(im, dtype=np.uint8).copy()


def box(a):
    p = np.pad(a, BOX // 2, mode="reflect")
    return sum(p[i:i + a.shape[0], j:j + a.shape[1]] for i in range(BOX) for j in range(BOX))


def shi_tomasi(img):
    p = np.pad(img.astype(np.float64), 1, mode="reflect")
    gx = p[1:-1, 2:] - p[1:-1, :-2]
    gy = p[2:, 1:-1] - p[:-2, 1:-1]
    a, b, c = box(gx * gx), box(gx * gy), box(gy * gy)
    r = 0.5 * (a + c) - np.sqrt(0.25 * (a - c) ** 2 + b * b)
    inside = np.zeros(r.shape, dtype=bool)
    inside[MARGIN:-MARGIN, MARGIN:-MARGIN] = True
    return np.where(inside, r, -1.0)


def keypoints(img):
    r = shi_tomasi(img)
    h, w = img.shape
    out = []
    for y0 in range(0, h, CELL):
        for x0 in range(0, w, CELL):
            cell = r[y0:y0 + CELL, x0:x0 + CELL]
            k = int(np.argmax(cell))
            cy, cx = divmod(k, cell.shape[1])
            if cell[cy, cx] > QUALITY * r.max():
                out.append((x0 + cx, y0 + cy))
    return np.array(out, dtype=np.float32)


def main(src):
    im1, im2 = read_gray(os.path.join(src, "1.png")), read_gray(os.path.join(src, "2.png"))
    np.savez_compressed(os.path.join(HERE, "flow_image_1.npz"), image=im1)
    np.savez_compressed(os.path.join(HERE, "flow_image_2.npz"), image=im2)
    kp = keypoints(im1)
    np.savez_compressed(os.path.join(HERE, "flow_keypoints.npz"), keypoints=kp)
    print("%d keypoints on %d x %d" % (len(kp), im1.shape[1], im1.shape[0]))


if __name__ == "__main__":
    main(sys.argv[1])
