// kt_rows.h — row lists of the pod feed calls.  Host only, no HIP: tests/cpp/unique_rows_test.cpp compiles this header alone.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace kt {

// The distinct rows of rows[0, n), ascending; *n_out is their number.  A list that is strictly ascending already — no entry, one
// entry, a sorted batch: what an informer usually hands over — is returned where it lies: the result is `rows` itself and `scratch`
// is not touched (no allocation).  Any other list is copied into `scratch`, sorted and made unique there; the result then points
// into `scratch` and lives as long as it does.
inline const int64_t* unique_rows(const int64_t* rows, int64_t n, std::vector<int64_t>& scratch, int64_t* n_out) {
  bool ascending = true;
  for (int64_t i = 1; i < n && ascending; ++i) ascending = rows[i] > rows[i - 1];
  if (ascending) {
    *n_out = n;
    return rows;
  }
  scratch.assign(rows, rows + n);
  std::sort(scratch.begin(), scratch.end());
  scratch.erase(std::unique(scratch.begin(), scratch.end()), scratch.end());
  *n_out = (int64_t)scratch.size();
  return scratch.data();
}

}  // namespace kt
