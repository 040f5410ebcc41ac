// Random finisher jobs for the stand-alone stress programs (nq_stack_stress.cpp,
// nq_split_stress.cpp): `row` queens on distinct columns, seen from row `row`.
#pragma once

#include <algorithm>
#include <array>
#include <cstdint>
#include <random>
#include <vector>

inline std::array<uint32_t, 4> random_job(std::mt19937& rng, int N, int rows) {
  const int row = N - rows;
  std::vector<int> colsv(N);
  for (int i = 0; i < N; i++) colsv[i] = i;
  std::shuffle(colsv.begin(), colsv.end(), rng);
  uint32_t cols = 0, d1 = 0, d2 = 0;
  for (int qr = 0; qr < row; qr++) {
    const int qc = colsv[qr];
    cols |= 1u << qc;
    const int a = qc + (row - qr), b = qc - (row - qr);
    if (a >= 0 && a < N) d1 |= 1u << a;
    if (b >= 0 && b < N) d2 |= 1u << b;
  }
  return {cols, d1, d2, static_cast<uint32_t>(row)};
}
