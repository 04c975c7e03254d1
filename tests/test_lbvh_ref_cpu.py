"""The plain LBVH restatement (tests/lbvh_ref.py) is itself a radix tree over strictly
increasing keys, on every scene the device build is compared with (test_lbvh.py).

The properties are checked from the definitions (Karras, HPG 2012, section 3), by brute
force over each node's key range, never with the helper's own split function.
"""
import numpy as np
import pytest

import lbvh_ref
import rtamd
from test_lbvh import check_structure

NAMES = sorted(lbvh_ref.SCENES)


def clz64(x):
    return 64 - int(x).bit_length()


@pytest.mark.parametrize("name", NAMES)
def test_reference_tree_is_a_tree_over_increasing_keys(name):
    fs = lbvh_ref.scene(name)
    nodes, indices, keys = lbvh_ref.reference(name)
    check_structure(rtamd.FlatScene(fs.shapes, nodes, indices, fs.camera, fs.light))
    k = [int(x) for x in keys]
    assert all(a < b for a, b in zip(k, k[1:])), "sorted keys must be strictly increasing"
    assert all(x >> 62 == 0 for x in k), "a key is 30 code bits over 32 index bits"
    assert [x & 0xffffffff for x in k] == indices.tolist()
    n = len(fs.shapes)
    assert (nodes["leftChild"][:n] == -1).all() and (nodes["rightChild"][:n] == -1).all()  # leaf j is node j
    assert (nodes["leftChild"][n:] >= 0).all()


@pytest.mark.parametrize("name", NAMES)
def test_reference_nodes_are_radix_tree_nodes(name):
    """For random inner nodes: every key in the node's range shares the prefix the range's
    first and last key share, the two children's ranges differ in the very next bit
    (all zeros left, all ones right), and each child sits where its range says: a leaf j
    at node j, an inner node at 2n-2 - (the end of its range next to the split)."""
    nodes, _, keys = lbvh_ref.reference(name)
    k = [int(x) for x in keys]
    n = len(k)
    rng = np.random.default_rng(5)
    inner = np.arange(n, 2 * n - 1)
    picks = set(rng.choice(inner, size=min(64, len(inner)), replace=False).tolist()) | {2 * n - 2, n}
    for me in sorted(picks):
        first = int(nodes["startShapeIdx"][me])
        last = first + int(nodes["numShapes"][me]) - 1
        assert 0 <= first < last < n
        karras = 2 * n - 2 - me
        assert karras in (first, last) and (me != 2 * n - 2 or (first, last) == (0, n - 1))
        p = clz64(k[first] ^ k[last])
        assert all(clz64(k[first] ^ k[j]) >= p for j in range(first, last + 1))
        # no wider range keeps that prefix: the node is the radix-tree node of the prefix
        assert first == 0 or clz64(k[first] ^ k[first - 1]) < p
        assert last == n - 1 or clz64(k[first] ^ k[last + 1]) < p
        L, R = int(nodes["leftChild"][me]), int(nodes["rightChild"][me])
        lf, ln = int(nodes["startShapeIdx"][L]), int(nodes["numShapes"][L])
        rf, rn = int(nodes["startShapeIdx"][R]), int(nodes["numShapes"][R])
        assert lf == first and rf == lf + ln and rf + rn - 1 == last
        bit = 63 - p  # the first bit below the shared prefix
        assert all((k[j] >> bit) & 1 == 0 for j in range(lf, rf))
        assert all((k[j] >> bit) & 1 == 1 for j in range(rf, last + 1))
        g = rf - 1
        assert L == (g if ln == 1 else 2 * n - 2 - g)
        assert R == (g + 1 if rn == 1 else 2 * n - 2 - (g + 1))


def test_reference_codes_on_known_points():
    """The quantisation and the bit order on centres whose codes are known by hand."""
    c = np.array([[0, 0, 0], [1, 1, 1], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.25, 0.125],
                  [np.inf, 0.5, 0.5], [0.5, np.nan, 0.5]], np.float32)
    code = [int(x) for x in lbvh_ref.morton_codes(c)]
    x_bits = sum(1 << (3 * b + 2) for b in range(10))
    assert code[0] == 0 and code[1] == (1 << 30) - 1
    assert code[2] == x_bits and code[3] == x_bits >> 1 and code[4] == x_bits >> 2
    # q = (512, 256, 128): one bit per axis, x at bit 9, y at bit 8, z at bit 7
    assert code[5] == (1 << (3 * 9 + 2)) | (1 << (3 * 8 + 1)) | (1 << (3 * 7))
    assert code[6] == 0 and code[7] == 0  # non-finite centres: cell 0, and outside the bounds
    same = np.array([[2, 3, 4]] * 3, np.float32)  # no extent: u = 0.5 on every axis
    assert [int(x) for x in lbvh_ref.morton_codes(same)] == [7 << 27] * 3
