"""What the CPU and GPU tests of `train_tgtcs --origin_train` share: the config and a fabricated LLFF scene directory."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FERN = os.path.join(ROOT, "configs", "fern.txt")


def llff_scene(base, n=3, h=6, w=8, factor=4):
    """A fabricated LLFF scene: poses_bounds.npy of n forward-facing cameras and images_<factor>/ of n h x w PNGs with
    distinct pixel values.  -> (directory, [uint8 images in file order])"""
    from PIL import Image
    rng = np.random.default_rng(7)
    os.makedirs(os.path.join(base, "images_%d" % factor))
    imgs = []
    for i in range(n):
        a = ((np.arange(h * w * 3).reshape(h, w, 3) * 5 + 37 * i) % 256).astype(np.uint8)
        Image.fromarray(a).save(os.path.join(base, "images_%d" % factor, "view_%02d.png" % i))
        imgs.append(a)
    rows = []
    for i in range(n):
        # LLFF layout [down, right, back | position | h, w, focal], cameras side by side looking down -z
        pose = np.concatenate([np.array([[0., 1., 0.], [-1., 0., 0.], [0., 0., 1.]]) + 0.01 * rng.standard_normal((3, 3)),
                               np.array([[0.3 * (i - 1)], [0.05 * i], [0.02 * i]]),
                               np.array([[h * factor], [w * factor], [0.9 * w * factor]])], 1)
        rows.append(np.concatenate([pose.reshape(15), [2.0, 9.0]]))
    np.save(os.path.join(base, "poses_bounds.npy"), np.stack(rows))
    return base, imgs
