// seg_layout.h -- the block behind a segment table of c segments (ctx_memory.hip owns it: a device copy, KB_SEG_TABLE, and a pinned
// host copy of the same room).  Plain arithmetic on c, in u64 words; tests/host_layer_check.cc holds it against the room.
//
//   [0, c+1)       the offsets (seg_table_set)
//   [c+1, 3c+3)    the region behind the table, which three users share:
//     upload       from c+1, at most 2c+1 words: a stage's second table on its way to the device (seg_upload_extra)
//     directory    [c+1, 3c+1), pinned copy only: the frame directory of pack / unpack, 16 bytes per block
//     read-back    from 2c+2, (c+1)/2 words, pinned copy only: the 32-bit values of a segmented checksum
//
// Who overlaps whom, and what must have drained before each is written (the host writes the pinned copy; copies on the context's
// stream read or write it):
//   * offsets: every call that sets a table drains the stream first, so no copy of an earlier table still reads the block;
//   * upload: lies on the directory and, from c+2 words on, on the read-back.  A stage writes it right behind its seg_table_set or
//     behind a drained stream: pack.hip drains between two stages so that no upload of the stage before is still to come;
//   * read-back: the checksum uploads c+1 words, which end where the read-back begins -- the one case where both are live;
//   * directory: written when every stage of the call has drained (pack), or read before the first stage runs and copied out of
//     the block at once (unpack): the stages' uploads and the checksum's read-back then go over it.
#pragma once

#include <stdint.h>

static inline uint64_t seg_offset_words(uint64_t c) { return c + 1; }
static inline uint64_t seg_upload_at(uint64_t c) { return c + 1; }
static inline uint64_t seg_upload_max_words(uint64_t c) { return 2 * c + 1; }
static inline uint64_t seg_dir_at(uint64_t c) { return c + 1; }
static inline uint64_t seg_dir_words(uint64_t c) { return 2 * c; }
static inline uint64_t seg_readback_at(uint64_t c) { return 2 * (c + 1); }
static inline uint64_t seg_readback_words(uint64_t c) { return (c + 1) / 2; }
// the room both copies are given: three times the offsets, rounded up to 64 KiB
static inline uint64_t seg_room_bytes(uint64_t c) { return (3 * seg_offset_words(c) * 8 + 65535) / 65536 * 65536; }
