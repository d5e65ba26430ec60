"""The cases of tests/test_work_order.py, checked without a GPU: that the numpy model of the work order's contract (tests/work_order_cases.py)
meets the conditions under which the device tests can see a fault, and that the sort's case list reaches the kernel's edges.  Every
count is printed (pytest -s)."""
import numpy as np

import work_order_cases as wc


def test_sort_cases_reach_the_edges_of_the_kernel():
    """The class arrays handed to rt_unit_tile_order_sort: every n of the issue with every pattern; among them an n whose last threads
    own no tile, an n with 64 or more tiles per thread, and all five classes in one array.  The model's order is a permutation."""
    ns, five, total = set(), 0, 0
    for label, a in wc.sort_cases():
        n = len(a)
        assert a.dtype == np.uint8 and n >= 1 and int(a.max()) < 5, label
        ns.add(n)
        five += len(np.unique(a)) == 5
        total += 1
        if n <= 5000:
            o = wc.stable_descending(a)
            assert np.array_equal(np.sort(o), np.arange(n)) and (np.diff(a[o].astype(np.int16)) <= 0).all(), label
            same = np.diff(a[o].astype(np.int16)) == 0
            assert (np.diff(o.astype(np.int64))[same] > 0).all(), label  # stable: equal classes keep the image order
    empty_tail = sorted(n for n in ns if wc.per_thread(n) * 1023 >= n)
    wide = sorted(n for n in ns if wc.per_thread(n) >= 64)
    print("%d sort cases over n = %s; last threads empty at n = %s; 64 or more tiles per thread at n = %s; %d arrays hold all five classes"
          % (total, sorted(ns), empty_tail, wide, five))
    assert ns == set(wc.SORT_NS)
    assert any(n > 1024 for n in empty_tail) and wide and five >= len(wc.SORT_NS) - 3  # (n = 1, 2 cannot hold five classes)


def test_scene_cases_cover_the_shapes_of_the_issue(built, oracle):
    from cpuraytracer_amd import _capi
    L = _capi.load()
    cs = [wc.case(oracle, k) for k in range(len(wc.CASES))]
    assert 10 <= len(cs) <= 14
    npix = [c.W * L.rt_rowset_local_rows(c.rs) for c in cs]
    assert any(c.W % 64 == 0 for c in cs) and any(c.W > 64 and c.W % 64 for c in cs) and any(c.W < 64 for c in cs)
    assert any(p % 64 == 0 for p in npix) and any(p % 64 for p in npix)
    assert any(c.rs.nshards == 1 and c.rs.num_rows == c.H for c in cs) and any(c.rs.nshards == 1 and c.rs.num_rows < c.H for c in cs)
    assert {(c.rs.nshards, c.rs.block_rows) for c in cs} >= {(3, 1), (3, 4)}
    assert any(c.sc.camera.aperture > 0 and c.sampler == 0 for c in cs) and any(c.sc.camera.aperture > 0 and c.sampler == wc.SQRT_DISK for c in cs)
    assert any(c.sc.camera.aperture == 0 for c in cs)
    assert {wc.CASES[c.k][0] for c in cs} == {"cover", "cap"}


def test_model_meets_the_honesty_conditions(built, oracle):
    """On the model alone: every stored class on at least 8 tiles of one case; the neighbour rule raises a tile -- one whose stored class
    shows it -- through each of its six pixels, and through each of them ALONE; a raised tile in the first tile row and one in the last;
    a tile left alone because its only glass neighbour is the partial tile; a flagged tile beside a glass tile; at least 5 tiles
    decided by the middle pilot alone and 5 by the last; no case with fewer than 3 distinct stored classes."""
    best = np.zeros(5, dtype=np.int64)
    through, alone_k = np.zeros(6, dtype=np.int64), np.zeros(6, dtype=np.int64)
    first = last = partial = beside = 0
    pilots = np.zeros(3, dtype=np.int64)
    for k in range(len(wc.CASES)):
        c, m = wc.case(oracle, k), wc.case_model(oracle, k)
        h = wc.honesty(c, m)
        print(c.label + ": %d full tiles" % m["n"])
        for name, v in h.items():
            print("    %s: %s" % (name, v))
        assert h["distinct stored classes"] >= 3, c.label
        assert np.array_equal(np.sort(m["order"]), np.arange(m["n"]))
        best = np.maximum(best, h["tiles per stored class"])
        through += h["raised through pixel k"]
        alone_k += h["raised through pixel k alone"]
        first += h["raised in the first tile row"]
        last += h["raised in the last tile row"]
        partial += h["not raised, the only glass neighbour is the partial tile"]
        beside += h["flagged beside a glass tile"]
        pilots += np.array(h["decided by the first, middle, last pilot alone"])
    print("over the cases: most tiles of one case per stored class %s; raised through pixel k %s, alone %s; first row %d, last row %d; "
          "partial-only %d; flagged beside glass %d; decided by one pilot alone %s" % (best, through, alone_k, first, last, partial, beside, pilots))
    assert (best >= 8).all(), best
    assert (through >= 1).all() and (alone_k >= 1).all(), (through, alone_k)
    assert first >= 1 and last >= 1 and partial >= 1 and beside >= 1
    assert pilots[1] >= 5 and pilots[2] >= 5, pilots


def test_model_without_flags_has_no_class_0_and_the_other_classes_unchanged(built, oracle):
    for k in range(len(wc.CASES)):
        m, m0 = wc.case_model(oracle, k), wc.case_model(oracle, k, False)
        assert (m0["classes"] >= 1).all() and not m0["flags"].any()
        keep = m["flags"] == 0
        assert np.array_equal(m["classes"][keep], m0["classes"][keep]) and np.array_equal(m0["classes"], m["after"] + 1)
