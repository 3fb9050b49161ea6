"""A plain restatement of cp_ccl_instance_labels' rule (include/casapose_hip.h) on top of ccl_reference.components, which labels every object's
binary map with SciPy: it shares nothing with the kernel's union-find, its keys or its passes.  Used only by the tests
(test_instance_reference.py pins it against hand-written maps on the CPU, test_gpu_ccl_instances.py compares the kernel with it).

The rule: a component is a 4-connected set of equal labels in 1..objects; it is eligible with at least min_size pixels; the eligible components
of an object are ordered by size descending, then root ascending (the root is the raster index of the component's first pixel); instance r
(0-based) of object o (1-based) gets slot (o-1)*R + r + 1; every other pixel gets slot 0."""
from types import SimpleNamespace

import numpy as np

import ccl_reference as R


def ranked(root_n, sizes, labels_n, objects):
    """{o: [(root, size)] of object o in one image, every component, ordered by (size descending, root ascending)}; roots are image-global"""
    roots = np.unique(root_n[root_n >= 0])
    h, w = labels_n.shape
    lab = labels_n.reshape(-1)[roots % (h * w)]
    out = {}
    for o in range(1, objects + 1):
        mine = roots[lab == o]
        out[o] = sorted(((int(r), int(sizes[r])) for r in mine), key=lambda c: (-c[1], c[0]))
    return out


def instance_labels(labels, objects, max_instances, min_size, components=None):
    """labels uint8 [b,h,w] -> (slots uint8 [b,h,w], inst int32 [b,objects,R,2] = (size, image-local root), (0, -1) for an empty slot).
    components: (root, sizes) of ccl_reference.components for these labels and objects, if the caller has them."""
    labels = np.asarray(labels)
    b, h, w = labels.shape
    hw = h * w
    assert 1 <= max_instances <= 16 and objects * max_instances <= 254
    root, sizes = components if components is not None else R.components(labels, objects)
    slot_of_root = np.zeros(b * hw, np.uint8)
    inst = np.zeros((b, objects, max_instances, 2), np.int32)
    inst[..., 1] = -1
    for n in range(b):
        for o, comps in ranked(root[n], sizes, labels[n], objects).items():
            eligible = [c for c in comps if c[1] >= min_size]
            for r, (rt, size) in enumerate(eligible[:max_instances]):
                slot_of_root[rt] = (o - 1) * max_instances + r + 1
                inst[n, o - 1, r] = (size, rt - n * hw)
    slots = np.where(root >= 0, slot_of_root[np.maximum(root, 0)], 0).astype(np.uint8)
    return slots, inst


# ---- hand-written maps with their expected results written out by hand ------------------------------------------------------------------------------
# 2 x 37 x 70 against the kernel's 64 x 16 tiles: W % 4 != 0, two tile columns (the second 6 wide), three tile rows (the last 5 high)
H, W = 37, 70
HW = H * W


def hand_edges():
    """objects 3, R 2, min_size 6.  Image 0: object 1 has components of 20, 12 and 12 pixels (more eligible ones than R; the tie in size goes
    to the smaller root), object 2 one of min_size - 1 and one of min_size, label 7 is above `objects`.  Image 1: object 3 covers more than half
    of the image."""
    lab = np.zeros((2, H, W), np.uint8)
    lab[0, 31:33, 10:20] = 1       # 20 pixels across the tile border y = 32, root 31 * 70 + 10
    lab[0, 2:5, 62:66] = 1         # 12 pixels across the tile border x = 64, root 2 * 70 + 62
    lab[0, 20:24, 60:63] = 1       # 12 pixels, root 20 * 70 + 60: the later of the tie, ranked third
    lab[0, 10, 0:5] = 2            # 5 pixels: not eligible
    lab[0, 12, 64:70] = 2          # 6 pixels in the ragged tile column, root 12 * 70 + 64
    lab[0, 15:18, 30:40] = 7       # above objects: background
    lab[1, 0:25, :] = 3            # 1750 of 2590 pixels
    slots = np.zeros_like(lab)
    slots[0, 31:33, 10:20] = 1
    slots[0, 2:5, 62:66] = 2
    slots[0, 12, 64:70] = 3
    slots[1, 0:25, :] = 5
    inst = np.array([[[[20, 2180], [12, 202]], [[6, 904], [0, -1]], [[0, -1], [0, -1]]],
                     [[[0, -1], [0, -1]], [[0, -1], [0, -1]], [[1750, 0], [0, -1]]]], np.int32)
    return SimpleNamespace(name="hand_edges", labels=lab, objects=3, max_instances=2, min_size=6, slots=slots, inst=inst)


def hand_254():
    """objects 127, R 2: objects * R = 254, the last slot id a byte can hold.  Object 127 has components of 3, 2 and 1 pixels, object 1 one of 4,
    object 64 two of 2 (the tie again); min_size 1."""
    lab = np.zeros((2, H, W), np.uint8)
    lab[0, 0, 0:3] = 127           # 3, root 0
    lab[0, 5, 68:70] = 127         # 2, root 5 * 70 + 68
    lab[0, 36, 69] = 127           # 1: the image's last pixel, ranked third
    lab[0, 16:18, 63:65] = 1       # 4 pixels around the tile corner (64, 16), root 16 * 70 + 63
    lab[1, 3, 3:5] = 64            # 2, root 3 * 70 + 3
    lab[1, 2, 40:42] = 64          # 2, root 2 * 70 + 40: the smaller root, ranked first
    slots = np.zeros_like(lab)
    slots[0, 0, 0:3] = 253
    slots[0, 5, 68:70] = 254
    slots[0, 16:18, 63:65] = 1
    slots[1, 2, 40:42] = 127
    slots[1, 3, 3:5] = 128
    inst = np.zeros((2, 127, 2, 2), np.int32)
    inst[..., 1] = -1
    inst[0, 126] = [[3, 0], [2, 418]]
    inst[0, 0, 0] = [4, 1183]
    inst[1, 63] = [[2, 180], [2, 213]]
    return SimpleNamespace(name="hand_254", labels=lab, objects=127, max_instances=2, min_size=1, slots=slots, inst=inst)


def hand_blocks():
    """3 x 48 x 136 (three tile columns, the last 8 wide; three full tile rows), objects 2, R 4, min_size 4: object 1 has six square blocks of 9,
    4, 16, 4, 25 and 1 pixels, so four instances in the order 25, 16, 9, 4 (the first 4-block in raster order) with one eligible block left over;
    object 2 has two; image 2 is empty."""
    lab = np.zeros((3, 48, 136), np.uint8)
    at = {9: (1, 1), 4: (14, 62), 16: (30, 126), 25: (40, 60), 1: (47, 135)}
    for size, (y, x) in at.items():
        s = int(round(size ** 0.5))
        lab[0, y:y + s, x:x + s] = 1
    lab[0, 20:22, 100:102] = 1     # the second block of 4 pixels, root 20 * 136 + 100
    lab[1, 15:17, 0:136] = 2       # 272 pixels across both tile borders in x and the one at y = 16
    lab[1, 40, 10:20] = 2          # 10
    slots = np.zeros_like(lab)
    for r, size in enumerate((25, 16, 9, 4)):
        y, x = at[size]
        s = int(round(size ** 0.5))
        slots[0, y:y + s, x:x + s] = r + 1
    slots[1, 15:17, 0:136] = 5
    slots[1, 40, 10:20] = 6
    inst = np.zeros((3, 2, 4, 2), np.int32)
    inst[..., 1] = -1
    inst[0, 0] = [[25, 40 * 136 + 60], [16, 30 * 136 + 126], [9, 1 * 136 + 1], [4, 14 * 136 + 62]]
    inst[1, 1, :2] = [[272, 15 * 136], [10, 40 * 136 + 10]]
    return SimpleNamespace(name="hand_blocks", labels=lab, objects=2, max_instances=4, min_size=4, slots=slots, inst=inst)


HAND = {"hand_edges": hand_edges, "hand_254": hand_254, "hand_blocks": hand_blocks}
