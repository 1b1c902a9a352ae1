"""The census of tests/tx_cases.py: the case lists of the transmit-side stage tests reach every path of the encoder, the
rate-matching kernel and the CRC staging helpers -- a condition on the inputs, checked without a GPU.  Each test fails with the
list of classes it misses, and dropping any one rate-matching or CRC set strands a class that the message names."""
import pytest

import tx_cases as T


def test_encoder_lists_reach_every_class():
    universe, reached = T.enc_universe(), T.enc_reached()
    assert not set(reached) - universe
    missing = sorted(universe - set(reached))
    assert not missing, "encoder classes (BG, NWC, Z %% 32 == 0, ring, copy, extension store) no (Z, offsets) reaches: %r" % missing
    # what the census is for: the ballot ring build at Z % 32 == 0 and the byte-wise stores at 4 | Z exist only at offset pointers
    aligned = T.enc_reached_from_aligned_bases()
    assert {c for c in universe if c[2] and c[3] != "words"} and not {c for c in aligned if c[2] and c[3] != "words"}
    assert not {c for c in aligned if c[1] == 4 and c[5] == "byte"}
    # a workgroup per codeword exists only with 16 | Z
    assert all(Z % 16 == 0 for Z in T.ALL_Z if T.enc_nwc(1, Z) == 4) and all(Z % 4 == 0 for Z in T.ALL_Z if Z > 48)
    for bg in (1, 2):
        for Z in T.ENC_SIZES[bg]:
            assert Z in T.ALL_Z
            per_wg = T.ENC_WAVES // T.enc_nwc(bg, Z)
            assert any(b % per_wg for b in T.enc_batches(bg, Z)) or per_wg == 1  # a ragged last workgroup
    assert {T.enc_class(bg, Z, 0, 0)[1:4] for bg, Z in T.ENC_RING_SIZES} | {T.enc_class(bg, Z, 1, 1)[1:4] for bg, Z in T.ENC_RING_SIZES} \
        == {c[1:4] for c in universe}


_ENC_CORE = {bg: tuple(Z for Z in T.ENC_SIZES[bg] if Z not in T.ENC_SIZES_FOR_SIZE[bg]) for bg in (1, 2)}


def test_encoder_sizes_kept_for_their_size_are_the_odd_and_the_largest():
    assert all(set(T.ENC_SIZES_FOR_SIZE[bg]) < set(T.ENC_SIZES[bg]) for bg in (1, 2))
    assert T.ENC_SIZES_FOR_SIZE[1][0] % 2 == 1 and T.ENC_SIZES_FOR_SIZE[1][1] == T.ENC_SIZES_FOR_SIZE[2][0] == max(T.ALL_Z)
    missing = sorted(T.enc_universe() - set(T.enc_reached(_ENC_CORE)))
    assert not missing, "encoder classes the sizes without ENC_SIZES_FOR_SIZE do not reach: %r" % missing


@pytest.mark.parametrize("bg,Z", [(bg, Z) for bg in (1, 2) for Z in _ENC_CORE[bg]])
def test_every_other_encoder_size_is_needed(bg, Z):
    rest = {b: tuple(z for z in _ENC_CORE[b] if (b, z) != (bg, Z)) for b in (1, 2)}
    stranded = sorted(T.enc_universe() - set(T.enc_reached(rest)))
    assert stranded, "BG%d Z = %d reaches no class of its own" % (bg, Z)


def test_rate_match_sets_reach_all_45_classes_and_both_stores():
    runs, stores = T.rm_universe()
    assert len(runs) == 45 and len(stores) == 10
    missing = T.rm_missing(T.RM_SETS)
    assert not missing, "rate-matching classes (Q_m, repetition, run) / stores / properties no set reaches: %r" % missing


@pytest.mark.parametrize("i", range(len(T.RM_SETS)))
def test_every_rate_match_set_is_needed(i):
    stranded = T.rm_missing(T.RM_SETS[:i] + T.RM_SETS[i + 1:])
    assert stranded, "set %d (%r) reaches nothing of its own" % (i, T.RM_SETS[i])


def test_rate_match_sets_have_the_derived_shapes_they_are_listed_for():
    refs = [T.derive(kw) for kw in T.RM_SETS]
    assert refs[0]["E_r"] == [1111, 1112, 1112] and T.rm_offsets(refs[0]) == [0, 1111, 2223]
    assert refs[1]["E_r"] == [1112, 0, 1112]
    assert refs[2]["Z_c"] == 384 and refs[2]["C"] == 1
    assert {r["Z_c"] for r in refs[3:]} == {6, 20} and all(r["G"] <= 310 and r["BG"] == 2 for r in refs[3:])
    # the two classes nothing reached before: Q_m = 1 with repetition across the buffer end, Q_m = 6 without repetition across the gap
    alone = [T.rm_census(r)[0] for r in refs]
    assert any((1, True, "wrapP") in a for a in alone) and any((6, False, "gap") in a for a in alone)


def test_crc_sets_reach_all_16_x_16_alignments_and_every_rotation():
    want = T.crc_universe()
    for call in ("attach", "check"):
        assert len({w for w in want if w[:2] == (call, "src,dst")}) == 256
        assert len({w for w in want if w[:2] == (call, "dst,rot")}) == 64 and len({w for w in want if w[:2] == (call, "rot")}) == 4
    missing = T.crc_missing(T.CRC_SETS)
    assert not missing, "CRC staging classes (call, src & 15, dst & 15) / (call, dst & 15, rotation) no set reaches: %r" % missing
    assert [T.derive(kw)["C"] for kw, _ in T.CRC_SETS] == [1, 2, 3, 5, 9, 1, 1, 1]
    for kw, n_tb in T.CRC_SETS[5:]:
        ref = T.derive(kw)
        assert ref["A"] % 2 == 1 and n_tb == 17 and {(t * ref["A"]) % 16 for t in range(n_tb)} == set(range(16))
    big, n_big = max(((T.derive(kw), n) for kw, n in T.CRC_SETS), key=lambda x: x[0]["C"] * x[0]["K"] * x[1])
    assert big["C"] == 9 and n_big == 2  # the largest single shape of the stage tests


@pytest.mark.parametrize("i", range(len(T.CRC_SETS)))
def test_every_crc_set_is_needed(i):
    stranded = T.crc_missing(T.CRC_SETS[:i] + T.CRC_SETS[i + 1:])
    assert stranded, "set %d (%r) reaches nothing of its own" % (i, T.CRC_SETS[i])
