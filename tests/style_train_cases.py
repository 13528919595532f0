"""What the CPU and GPU tests of `train_tgtcs --style_train` share: the fabricated inputs of the reference's layout."""
import os

import numpy as np


def write_stylized_data(style_dir, styles=1, h=6, w=8):
    """stylized_gen_<factor>/stylized_data.npz as the 2-D pass leaves it (trans_test.read_stylized_data reads it back)."""
    os.makedirs(style_dir, exist_ok=True)
    rng = np.random.default_rng(5)
    names = {"style_%d" % i: i for i in range(styles)}
    np.savez(os.path.join(style_dir, "stylized_data.npz"), style_names=np.array(names, dtype=object),
             style_paths=np.array([style_dir + "/"] * styles), style_images=rng.random((styles, h, w, 3)).astype(np.float32),
             style_features=rng.standard_normal((styles, 1024)).astype(np.float32))


def style_inputs(datadir, gen_path, n=3, h=6, w=8, factor=4.0, rendered=None):
    """Beside an origin_train_cases.llff_scene: <gen_path>/rgb_%05d.png (written here unless `rendered`: then --render_train
    wrote them), <datadir>/stylized_gen_<factor>/NNN.jpg from 001 and stylized_data.npz.
    -> ([uint8 rgb_origin frames as written], [uint8 stylised frames as a JPEG decoder returns them])"""
    from PIL import Image
    style_dir = os.path.join(datadir, "stylized_gen_" + str(factor))
    write_stylized_data(style_dir, 1, h, w)
    origin, stylised = [], []
    if not rendered:
        os.makedirs(gen_path, exist_ok=True)
    for i in range(n):
        if not rendered:
            a = ((np.arange(h * w * 3).reshape(h, w, 3) * 3 + 91 * i) % 256).astype(np.uint8)
            Image.fromarray(a).save(os.path.join(gen_path, "rgb_%05d.png" % i))
            origin.append(a)
        yy, xx = np.mgrid[0:h, 0:w]
        b = np.stack([(xx * 29 + 40 * i) % 256, (yy * 37 + 11) % 256, ((xx + yy) * 13 + 70 * i) % 256], -1).astype(np.uint8)
        path = os.path.join(style_dir, "%03d.jpg" % (i + 1))
        Image.fromarray(b).save(path, quality=95)
        stylised.append(np.array(Image.open(path).convert("RGB"), np.uint8))
    return origin, stylised
