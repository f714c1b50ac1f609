"""MI355X-native approximate k-mer counter (drop-in for qbonenfant/approx_counter's
approximate-count stage, ``errorCount`` at approx_counter.cpp:531-601).

The compute path is the HIP kernel behind the C ABI in
include/approx_counter_amd.h; this package is the host-side mirror of the
reference interface for that path (see counter.error_count).
"""
from .counter import (ApproxCounter, DeviceSegment, Dna5Sample, Jobs, PackedSample, WindowHits, cooccurrence_words,
                      cross_cooccurrence_words,
                      distances_from_hits, edit_consensus, edit_words, flank_consensus, flank_words,
                      error_count, error_levels, hits_words, pack_windows, pinned_copy, pinned_empty, positions_words,
                      to_dna5, unpack_hits, unpack_positions, unpack_starts)
from ._lib import ApproxCounterError

__all__ = ["ApproxCounter", "ApproxCounterError", "DeviceSegment", "Dna5Sample", "Jobs", "PackedSample", "WindowHits",
           "cooccurrence_words", "cross_cooccurrence_words", "distances_from_hits", "edit_consensus", "edit_words", "flank_consensus", "flank_words", "error_count", "error_levels", "hits_words", "pack_windows", "pinned_copy",
           "pinned_empty", "to_dna5", "unpack_hits", "positions_words", "unpack_positions", "unpack_starts"]
