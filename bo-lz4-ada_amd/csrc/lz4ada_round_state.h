// lz4ada_round_state.h -- the reference's Output_Pos / Output_Pos_History
// (lz4ada.adb:678-690, 785-787), stated once for every host unit, and the
// flags that carry quirk D1 between the host and the decoders.  Standard
// library only, so a plain C++ program can include it
// (tools/linked_accept_check.cpp); lz4ada_internal.h includes it for the
// kernel files, whose own statements of the rule (decode_chain in
// lz4ada_idx.hip, the serial kernel in lz4ada_kernels.hip, on SerialState)
// stay where they are.
#pragma once
#include <stdint.h>

namespace lz4ada {

constexpr int64_t HISTORY_SIZE = 65536;  // lz4ada.ads:350

// Quirk D1: the reference's 8-byte wild copy (lz4ada.adb:811-817) may
// clobber history bytes [Output_Pos + 1, Output_Pos + 7] before a match
// reads them; that needs Output_Pos_History in [65536, 65542] and an offset
// >= Output_Pos_History - 7 >= D1_OFF.  The decoders flag every block with
// such a match reaching before its start (status aux bit AUX_D1_RISK on a
// DS_OK block) and the host sends those frames to the exact path.
constexpr int32_t D1_OFF = int32_t(HISTORY_SIZE) - 7;
constexpr int32_t AUX_D1_RISK = 1;
// Quirk D1 in the linked bulk path, emulated (round 6): the host predicts
// each block's round state from the slot sizes (every block full) and
// passes it in the descriptor's flags -- BLOCK_D1_ROUND: the block's round
// follows one that ended at Output_Pos_History = 65536 + the 3 bits at
// BLOCK_D1_OPH_SHIFT; bits from BLOCK_N1_SHIFT: Output_Pos at the block's
// start (its place in the round).  The index decoder then writes a D1
// match's first bytes as the reference's wild literal copy leaves them
// (lz4ada.adb:811-817, 862-879; the lone decoder's k_lone_words does the
// same); its status carries AUX_D1_EMU (decoded under a prediction), and
// the host accepts such a block only if the real round state equals the
// prediction.  (Bits 0-1 are the public flags.)
constexpr uint32_t BLOCK_D1_ROUND = 8u;
constexpr int BLOCK_D1_OPH_SHIFT = 4;
constexpr int BLOCK_N1_SHIFT = 16;
constexpr int32_t AUX_D1_EMU = 4;
// the linked path's literal-zero decode (k_decode_idx_zl): a match reads
// history positions below 256, whose high byte is 0 like a literal's
constexpr int32_t AUX_DEEP_HIST = 2;

// Where the next block's output goes in the reference's Buffer, and where the
// last round ended.  Blocks form rounds: a block starts at Buffer position 0
// once the position has reached 64 KiB (:678-680) and appends otherwise; the
// history position follows the position whenever that has reached 64 KiB
// (:688-690 for stored blocks, :785-787).
struct RoundState {
	int64_t pos = 0;      // Ctx.Output_Pos
	int64_t history = 0;  // Ctx.Output_Pos_History
	// where the next block starts, the state left as it is (a block some
	// decoder may still decline)
	int64_t next_start() const { return pos >= HISTORY_SIZE ? 0 : pos; }
	// the next block's start, taken: a new round begins at 0
	int64_t start() { return pos = next_start(); }
	// the block that started at start() decoded to len bytes
	void advance(int64_t len)
	{
		pos += len;
		if (pos >= HISTORY_SIZE)
			history = pos;
	}
	// Quirk D1 can only strike right after a round that ended within the
	// reference's 8-byte wild copy of 64 KiB (lz4ada.adb:811-817, 862-879).
	bool in_d1() const { return history >= HISTORY_SIZE && history <= HISTORY_SIZE + 6; }
};

}  // namespace lz4ada
