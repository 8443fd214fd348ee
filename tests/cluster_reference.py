"""The scipy reference of the cluster sampler (md_cluster_*), shared by tests/test_clusters.py (hand-made graphs) and
tests/test_gpu_clusters.py (the device against it).  Nothing here comes from the code under test: the components are
scipy.sparse.csgraph.connected_components on a given pair list, everything else is numpy on its labels."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components


def clusters(n, pairs, member=None, max_size=1024):
    """The contract of include/mdhip.h for the unordered bonded pairs (a, b) among n particles; `member` (bool[n], default
    everyone) restricts the graph: a pair counts only if both ends are members.  Returns a dict: label[n] (the smallest
    particle id of the cluster, -1 for a non-member), size[n] (0 for a non-member), sizes (one per cluster, by ascending
    label), labels (those labels), fr[8] and hist[max_size + 1]."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    member = np.ones(n, dtype=bool) if member is None else np.asarray(member, dtype=bool)
    assert member.shape == (n,)
    assert not np.any(pairs[:, 0] == pairs[:, 1])
    pairs = pairs[member[pairs[:, 0]] & member[pairs[:, 1]]]
    graph = coo_matrix((np.ones(len(pairs), dtype=np.int8), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
    _, comp = connected_components(graph, directed=False)
    # canonical label: the smallest id of the component (over members; a non-member is a component of its own here)
    ids = np.arange(n, dtype=np.int64)
    smallest = np.full(comp.max() + 1 if n else 0, n, dtype=np.int64)
    np.minimum.at(smallest, comp, ids)
    label = np.where(member, smallest[comp], -1)
    labels, sizes = np.unique(label[member], return_counts=True)
    size = np.zeros(n, dtype=np.int64)
    if len(labels):
        size[member] = sizes[np.searchsorted(labels, label[member])]
    fr = np.zeros(8, dtype=np.int64)
    fr[0] = np.count_nonzero(member)
    fr[1] = len(sizes)
    fr[6] = -1
    if len(sizes):
        order = np.lexsort((labels, -sizes))                # by descending size, then ascending label
        fr[2] = sizes[order[0]]
        fr[3] = sizes[order[1]] if len(sizes) > 1 else 0
        fr[6] = labels[order[0]]
    fr[4] = 2 * len(pairs)
    fr[5] = int((sizes.astype(np.int64) ** 2).sum())
    fr[7] = np.count_nonzero(sizes == 1)
    return dict(label=label.astype(np.int64), size=size, sizes=sizes.astype(np.int64), labels=labels, fr=fr,
                hist=size_histogram(sizes, max_size))


def size_histogram(sizes, max_size):
    """hist[min(s, max_size)] += 1 for every cluster size s: max_size + 1 entries, entry 0 stays 0."""
    return np.bincount(np.minimum(np.asarray(sizes, dtype=np.int64), max_size), minlength=max_size + 1).astype(np.int64)
