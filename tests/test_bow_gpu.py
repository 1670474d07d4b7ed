"""The loop-closure candidate search on the GPU (k_bow.hip through the Python mirror) against
tests/bow_ref.py: word ids and counts as integers, every double by its bits."""
import numpy as np
import pytest

import bow_cases as BC
import bow_ref as R
import gfpl
import loop_closure_cases as LC

pytestmark = pytest.mark.gpu

VOCABS = BC.vocabularies()
BATCH_SIZES = (5, 63, 1, 64, 0, 257, 3, 65)   # eight sets of unequal counts, an empty one in the middle


@pytest.fixture(scope="module")
def ctx():
    cam, cfg = LC.setup()
    c = gfpl.Context(cam, cfg)
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def make_voc(ctx, v):
    return gfpl.Vocabulary(ctx, v["child_off"], v["child"], v["desc"], v["weight"], v["word_id"], v["weighting"], v["scoring"])


def assert_vectors(got, ref, what):
    assert len(got) == len(ref)
    for k, ((ids, vals), r) in enumerate(zip(got, ref)):
        assert ids.dtype == np.int32 and vals.dtype == np.float64
        assert ids.tolist() == [i for i, _ in r], (what, k)
        assert [R.bits(x) for x in vals] == [R.bits(x) for _, x in r], (what, k)


@pytest.mark.parametrize("name", sorted(VOCABS))
def test_transform_batch(ctx, name):
    v = VOCABS[name]
    sets = BC.descriptor_sets(v, 100, sizes=BATCH_SIZES, sparse=name in ("ragged", "dup_siblings", "k17_L2", "k32_L2"))
    voc = make_voc(ctx, v)
    try:
        got = ctx.bowTransform(voc, [dev(s) for s in sets])   # cap = the largest count
        assert_vectors(got, BC.ref_transform(v, sets), name)
        for alone in (sets[1], sets[0][:4], sets[4]):   # one set per call: 63, 4 and 0 descriptors
            assert_vectors(ctx.bowTransform(voc, [dev(alone)]), BC.ref_transform(v, [alone]), name + " alone")
    finally:
        voc.close()


def test_transform_2000(ctx):
    v = VOCABS["k10_L3"]
    rng = np.random.default_rng(7)
    big = BC.descriptor_sets(v, 101, sizes=(2000,))[0]
    same = np.repeat(rng.integers(0, 256, (1, 32), dtype=np.uint8), 2000, axis=0)   # one word, 1999 additions
    tenth = VOCABS["tenth"]
    voc, voc10 = make_voc(ctx, v), make_voc(ctx, tenth)
    try:
        got = ctx.bowTransform(voc, [dev(big), dev(same), dev(big[:1999])])
        ref = BC.ref_transform(v, [big, same, big[:1999]])
        assert_vectors(got, ref, "2000")
        assert len(ref[1]) == 1 and len(ref[0]) > 500
        # a weight of 0.1 met many times: the sum of the additions, not a product
        few = np.concatenate([same[:10], big[:40]])
        got = ctx.bowTransform(voc10, [dev(few), dev(same)])
        assert_vectors(got, BC.ref_transform(tenth, [few, same]), "tenth")
    finally:
        voc.close()
        voc10.close()


def test_transform_stop_words_capacity_and_empty_call(ctx):
    v = VOCABS["all_stopped"]
    voc = make_voc(ctx, v)
    try:
        sets = BC.descriptor_sets(v, 102, sizes=(65, 4))
        got = ctx.bowTransform(voc, [dev(s) for s in sets])
        assert [len(i) for i, _ in got] == [0, 0]
        assert ctx.bowTransform(voc, []) == []
        with pytest.raises(gfpl.GfplError) as e:
            ctx.bowTransform(voc, [dev(sets[0]), dev(sets[1])], cap=64)   # 65 rows
        assert e.value.code == -5
        got = ctx.bowTransform(voc, [dev(sets[1])], cap=64)
        assert [len(i) for i, _ in got] == [0]
    finally:
        voc.close()


def test_context_refuses_to_close_while_a_vocabulary_lives():
    cam, cfg = LC.setup()
    c = gfpl.Context(cam, cfg)
    voc = make_voc(c, VOCABS["k2_L2"])
    db = gfpl.BowDatabase(c, voc, None, gfpl.BOW_MODE_P, 4, 8, 0)
    with pytest.raises(gfpl.GfplError):
        c.close()
    db.close()
    with pytest.raises(gfpl.GfplError):
        c.close()
    voc.close()
    c.close()


def test_scores(ctx):
    pairs = BC.score_pairs()
    names = sorted(pairs)
    got = ctx.bowScore([pairs[n][0] for n in names], [pairs[n][1] for n in names])   # one batch of mixed lengths
    for n, g in zip(names, got):
        assert R.bits(g) == R.bits(BC.ref_score(*pairs[n])), n
    for n in ("empty_empty", "empty_a", "a_empty", "disjoint"):
        assert R.bits(got[names.index(n)]) == 0x8000000000000000, n
    assert got[names.index("one_word_self")] == 1.0
    for n in ("nested", "runs", "len2000"):   # and alone
        assert R.bits(ctx.bowScore([pairs[n][0]], [pairs[n][1]])[0]) == R.bits(BC.ref_score(*pairs[n])), n
    assert len(ctx.bowScore([], [])) == 0


FILL = 7.25   # what the caller's row holds before an insert


@pytest.mark.parametrize("mode", ["P", "L", "PL"])
def test_database_sequence(ctx, mode):
    cam, _ = LC.setup()
    A, B = 10, 32
    f0, f1 = LC.make_pair(cam, BC.SEQ_PT, BC.SEQ_LS, seed=77)
    seq = BC.keyframe_sequence((A, B, f0, f1))
    vp, vl = VOCABS["k10_L3"], VOCABS["shuffled_words"]
    voc_p = make_voc(ctx, vp) if "P" in mode else None
    voc_l = make_voc(ctx, vl) if "L" in mode else None
    gmode = {"P": gfpl.BOW_MODE_P, "L": gfpl.BOW_MODE_L, "PL": gfpl.BOW_MODE_PL}[mode]
    db = gfpl.BowDatabase(ctx, voc_p, voc_l, gmode, BC.SEQ_N, BC.SEQ_PT, BC.SEQ_LS)
    ref = R.Database(BC.ref_vocab(vp), BC.ref_vocab(vl), mode)
    conf = np.zeros((BC.SEQ_N, BC.SEQ_N), np.float32)   # the reference's vector<vector<float>> conf_matrix
    alive = np.zeros(BC.SEQ_N, np.uint8)
    decisions = []
    try:
        for i, (pd, ld, pl, spl, epl) in enumerate(seq):
            stats = gfpl.bowStats(pl, spl, epl)
            rstats = R.bow_stats(pl, spl, epl)
            row = np.full(i + 1, FILL)
            dp, dl = dev(pd), dev(ld)
            if mode == "P":
                db.insertKFBowVectorP(i, row=row, pdesc=dp)
            elif mode == "L":
                db.insertKFBowVectorL(i, row=row, ldesc=dl)
            else:
                db.insertKFBowVectorPL(i, stats=stats, row=row, pdesc=dp, ldesc=dl)
            want = ref.insert(i, list(pd), list(ld), rstats)
            for j in range(i + 1):
                assert R.bits(row[j]) == R.bits(want.get(j, FILL)), (mode, i, j)
            if i == 0:
                assert row[0] == 1.0
            alive[i] = 1
            for j, s in want.items():
                conf[j, i] = conf[i, j] = s
            # the stored vectors are what bowTransform returns
            if i in (0, 5, A, B):
                if "P" in mode:
                    again = [list(zip(a.tolist(), b.tolist())) for a, b in ctx.bowTransform(voc_p, [dp])]
                    assert_vectors([db.vector(0, i)], again, "stored P")
                    assert_vectors([db.vector(0, i)], [ref.kf[i][0]], "stored P vs ref")
                if "L" in mode:
                    assert_vectors([db.vector(1, i)], [ref.kf[i][1]], "stored L vs ref")
            g = BC.graph_col(i)
            col = conf[:i, i].astype(np.float64)
            r = R.look_for_loop_candidates(col, alive, g, i, BC.SEQ_SEARCH)
            ok, prev, info = gfpl.lookForLoopCandidates(col, alive, g, i, gfpl.LcSearchParams(**BC.SEQ_SEARCH))
            assert (ok, prev, info.nkf_closest, info.idx_max, info.n_list, R.bits(info.lc_min_score)) == (
                r[0], r[1], r[2]["nkf_closest"], r[2]["idx_max"], r[2]["n_list"], R.bits(r[2]["lc_min_score"])), (mode, i)
            decisions.append((ok, prev))
            if i in BC.SEQ_ERASE:
                db.erase(BC.SEQ_ERASE[i])
                ref.erase(BC.SEQ_ERASE[i])
                alive[BC.SEQ_ERASE[i]] = 0
        assert decisions[B] == (True, A), decisions
        with pytest.raises(gfpl.GfplError):
            db.insert(3, pdesc=dev(seq[3][0]), ldesc=dev(seq[3][1]), stats=gfpl.bowStats(*seq[3][2:]))   # not new
        with pytest.raises(gfpl.GfplError):
            db.vector(0 if "P" in mode else 1, 7)   # erased
        if mode == "PL":
            # the two halves meet: the candidate the search names passes the device's loop-closure check
            res = ctx.isLoopClosure(gfpl.KeyFrameView(f0, np.eye(4), "cuda"), gfpl.KeyFrameView(f1, np.eye(4), "cuda"))
            assert res[0][0].is_lc == 1 and res[0][0].n_pt > BC.SEQ_PT // 2
    finally:
        db.close()
        for v in (voc_p, voc_l):
            if v is not None:
                v.close()
