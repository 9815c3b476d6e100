"""The four per-hit families share one set of buffers (hit table, partials, flags, results, pinned side, staged spans)
and one call frame: their calls interleaved, host and device forms in turn, each shared buffer sized by a small record
first and growing afterwards, every result bit for bit what the family gave on its own."""
import numpy as np
import pytest

import hit_bands_ref as bref
import hit_segments_ref as sref
import hit_significance_ref as gref
import test_gpu_hit_scores as hs
import test_gpu_hit_significance as hg

pytestmark = pytest.mark.gpu

S, N = 9001, 50_000
HITS = [0, 12_000, 12_500, N - S]
M, R, LF, NB, G, B = 5, 3, 10, 16, 64, 2000


@pytest.fixture(scope="module")
def alone(gpu):
    """Needle, haystack, parameters and each family's records of HITS from one call of its own, checked against its checker."""
    am = gpu
    needle, hay = hs.noise(71, S, 0.5), hs.noise(72, N, 0.1)
    for t in HITS:
        hay[t:t + S] += needle
    algo = hg.make_algo(am, needle)
    pk = hg.peaks_at(am, HITS)
    bp16, bp2 = am.band_edges_log(8000, LF, 100.0, 4000.0, NB), am.band_edges_log(8000, LF, 100.0, 4000.0, 2)
    base = {"scores": algo.hit_scores(hay, pk), "segments": algo.hit_segments(hay, pk, M, R), "bands": algo.hit_bands(hay, pk, bp16),
            "bands2": algo.hit_bands(hay, pk[:1], bp2), "significance": algo.hit_significance(hay, pk, G, B)}
    for i, t in enumerate(HITS):
        hs.assert_ref(base["scores"][i], hs.hit_ref(hay, needle, t))
        sref.assert_records(base["segments"][i], sref.segments_ref(hay, needle, t, M, R))
        bref.assert_records(base["bands"][i], bref.bands_ref(hay, needle, t, LF, list(bp16.edges[:NB + 1])))
        gref.assert_record(base["significance"][i], hg.library_ref(am, algo, hay, t, G, B))
    bref.assert_records(base["bands2"][0], bref.bands_ref(hay, needle, HITS[0], LF, list(bp2.edges[:3])))
    return algo, hay, pk, bp16, bp2, base


def test_interleaved_calls_keep_their_bits(gpu, alone):
    am = gpu
    algo, hay, pk, bp16, bp2, base = alone
    want = {"scores": hs.bits(base["scores"]), "segments": [sref.bits(q) for q in base["segments"]],
            "bands": [bref.bits(q) for q in base["bands"]], "bands2": [bref.bits(q) for q in base["bands2"]],
            "significance": hg.bits(base["significance"])}
    assert am.lib().am_shutdown() == am.AM_OK   # every shared buffer starts empty again
    buf = am.DeviceBuffer.from_numpy(0, hay)
    try:
        assert [bref.bits(q) for q in algo.hit_bands(hay, pk[:1], bp2)] == want["bands2"]                      # 1
        assert hs.bits(algo.hit_scores_device(buf.ptr, N, pk)) == want["scores"]                                # 2
        assert [sref.bits(q) for q in algo.hit_segments(hay, pk, M, R)] == want["segments"]                    # 3
        assert hg.bits(algo.hit_significance_device(buf.ptr, N, pk, G, B)) == want["significance"]              # 4
        assert [bref.bits(q) for q in algo.hit_bands(hay, pk, bp16)] == want["bands"]                          # 5
        assert hs.bits(algo.hit_scores_device(buf.ptr, N, pk[:1])) == want["scores"][:1]                        # 6
        both = am.hit_segments_batch_device([algo, algo], [buf.ptr], [N], [[pk, pk]], M, R)                   # 7
        assert [[sref.bits(q) for q in both[0][j]] for j in range(2)] == [want["segments"]] * 2
        assert hs.bits(algo.hit_scores(hay, pk)) == want["scores"]                                              # 8
    finally:
        buf.free()
