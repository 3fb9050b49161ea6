"""A plain restatement of cp_ccl_filter_labels (csrc/ccl.hip) that shares nothing with the kernel's method, used only by the tests
(test_ccl_reference.py on the CPU against the oracle, test_gpu_ccl_stages.py against the kernel's intermediate products): scipy labels every
object's binary map on its own, the selection rule is the sorted histogram of voting_layers_2d.py:64-76 written out."""
import numpy as np
from scipy import ndimage


def components(labels, objects):
    """labels uint8 [b,h,w] -> (root, sizes).  root int64 [b,h,w]: the image-global raster index (n*h*w + y*w + x) of the first pixel in raster
    order of the pixel's 4-connected component of equal labels; -1 on background and on labels above `objects`.  sizes int64 [b*h*w]: the pixel
    count of the component at every root index, 0 elsewhere."""
    labels = np.asarray(labels)
    b, h, w = labels.shape
    hw = h * w
    root = np.full((b, hw), -1, np.int64)
    sizes = np.zeros(b * hw, np.int64)
    for n in range(b):
        for o in np.unique(labels[n]):
            if o == 0 or o > objects:
                continue
            ids, k = ndimage.label(labels[n] == o)          # default structure: the 4-neighbourhood
            flat = ids.ravel()
            uniq, first = np.unique(flat, return_index=True)  # first[j]: the smallest raster index that carries id uniq[j]
            lut = np.zeros(k + 1, np.int64)
            lut[uniq] = first + n * hw
            on = flat > 0
            root[n, on] = lut[flat[on]]
            sizes[lut[1:]] = np.bincount(flat, minlength=k + 1)[1:]
    return root.reshape(b, h, w), sizes


def object_components(root_n, sizes, labels_n, o):
    """[(root, size)] of object o (1-based) in one image, in raster order of the first pixel"""
    r = np.unique(root_n[(labels_n == o) & (root_n >= 0)])
    return [(int(x), int(sizes[x])) for x in r]


def select(sizes_of_object, hw, min_size, rank):
    """The histogram {bin 0: hw - foreground, bin i: i-th component in raster order of its first pixel} of one (image, object), padded with empty
    bins to rank + 1 entries, bins below min_size zeroed, ordered by (count descending, index ascending): entry `rank` as (which, thresholded
    count) with which = "bin0", the component's root, or None for a padding bin.  sizes_of_object: [(root, size)]."""
    comps = sorted(sizes_of_object)
    who = ["bin0"] + [r for r, _ in comps]
    counts = [hw - sum(s for _, s in comps)] + [s for _, s in comps]
    while len(counts) < rank + 1:
        who.append(None)
        counts.append(0)
    counts = np.asarray(counts, np.int64)
    counts = np.where(counts < min_size, 0, counts)
    order = np.lexsort((np.arange(counts.size), -counts))
    k = int(order[rank])
    return who[k], int(counts[k])


def filter(labels, objects, min_size, rank):   # noqa: A001  (the name the kernel's entry point carries)
    """The kept label map: per (image, object) the pixels of the selected component, nothing where the selection is bin 0 or a padding bin."""
    labels = np.asarray(labels)
    b, h, w = labels.shape
    root, sizes = components(labels, objects)
    out = np.zeros_like(labels)
    for n in range(b):
        for o in np.unique(labels[n]):
            if o == 0 or o > objects:
                continue
            which, _ = select(object_components(root[n], sizes, labels[n], o), h * w, min_size, rank)
            if which is not None and which != "bin0":
                out[n][root[n] == which] = o
    return out
