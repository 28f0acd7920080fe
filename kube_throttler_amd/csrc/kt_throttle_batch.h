// kt_throttle_batch.h — the one validator of throttle batches (kt_throttle_batch.cpp): kt_upsert_throttles, kt_upsert_throttle and
// kt_load_snapshot run it over the whole batch before anything is stored; kt_validate_throttles exports it without an engine.
// Host code only: no HIP header, no engine object (tests/cpp/throttle_batch_test.cpp compiles the translation unit on its own).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/kt_engine.h"

namespace kt {

// KT_OK, or the code a feed call answers for this batch with the text kt_last_error gives in err[0, err_len) (always terminated).
// Reads nothing beyond what the counts and the offsets it has already checked cover; the value arrays of the requirement pools
// (kt_reqs.val) and the amounts' values are not read at all / only where a presence bit below n_dims names them.
__attribute__((visibility("hidden"))) int32_t validate_throttle_batch(const kt_snapshot* b, const int32_t* rows, int32_t n_dims, int32_t throttle_capacity,
                                int32_t namespace_capacity, char* err, size_t err_len);

}  // namespace kt
