"""The headline unit (BG1 Z = 384, split form) compiles from nrldpc_decode_z64q_inst.hip and nrldpc_decode_z64_pair.h, two files
outside build.kernel_id(): the ten sources that id hashes are unchanged, so the id did not move although the kernel did.  The
committed profile summaries that bench.py divides by therefore carry a second id, build.pair_search_id(), and this test holds
them to the tree: an edit of either file without a profile refresh fails here."""
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUMMARIES = ("r06_bench_pmc_summary.json", "r06_traffic_bytes_per_launch.json", "r06_headline_isa_mix.json")


def _load(name):
    return json.load(open(os.path.join(ROOT, "profiles", name)))


def test_profile_summaries_belong_to_the_paired_search_in_the_tree(pkg):
    bld = pkg._capi._build
    for name in SUMMARIES:
        assert _load(name)["_pair_search_id"] == bld.pair_search_id(), name


def test_kernel_id_is_the_summaries_and_the_frozen_sources_are_unchanged(pkg):
    """kernel_id() hashes the ten frozen files and the flags: equal to the id the summaries were collected under means none of
    them changed."""
    bld = pkg._capi._build
    pmc, traffic, mix = (_load(n) for n in SUMMARIES)
    assert bld.kernel_id() == pmc["_nrldpc_kernel_id"] == traffic["nrldpc_kernel_id"] == mix["nrldpc_kernel_id"]


def test_headline_size_is_built_from_the_paired_search(pkg):
    bld = pkg._capi._build
    assert (1, 384) in bld.Z64_PAIR
    assert bld.NOPAIR or bld.z64_source(1, 384) == bld.Z64Q_SOURCE != bld.Z64_SOURCE
    assert bld.z64_source(2, 384) == bld.Z64_SOURCE  # a size that has not been measured keeps the plain file
    for f in (bld.Z64Q_SOURCE, bld.Z64Q_HEADER):
        assert os.path.exists(os.path.join(bld.CSRC, f)) and os.path.join(bld.CSRC, f) in bld._deps()
    assert bld.Z64Q_HEADER in bld.HEADERS and not {bld.Z64Q_SOURCE, bld.Z64Q_HEADER} & set(bld.KERNEL_SOURCES)
    assert _load("r06_headline_isa_mix.json")["instantiation_file"] == bld.Z64Q_SOURCE  # the priced loop is the shipped unit's
