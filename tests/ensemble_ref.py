"""numpy restatement of the reference's ensembling (ensembling/ensemble.py:16-44) that the ensembling tests compare the
device against: the float32 average in member order and LabelManager.convert_logits_to_segmentation applied to it."""
import numpy as np


def average(members):
    """average_probabilities: p_0 as float32, += p_i in order, /= n."""
    avg = np.array(members[0], dtype=np.float32)
    for p in members[1:]:
        avg += p
    avg /= len(members)
    return avg


def sigmoid(x):
    x = np.asarray(x, np.float32)
    return np.float32(1) / (np.float32(1) + np.exp(-x))


def merge_rule(avg, regions_class_order=None):
    """convert_logits_to_segmentation on the average: argmax (first maximum wins), or - for regions - the sigmoid applied
    again to the averaged probabilities, > 0.5, painted in regions_class_order."""
    if regions_class_order is None:
        return avg.argmax(0)
    seg = np.zeros(avg.shape[1:], np.uint16)
    s = sigmoid(avg)
    for i, c in enumerate(regions_class_order):
        seg[s[i] > 0.5] = c
    return seg
