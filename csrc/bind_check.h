// Host-side operand checks shared by the binding files (bindings.cpp, comm_bind.cpp): every check
// runs BEFORE a launch, so a kernel never sees an operand its loads do not assume.
#pragma once
#include <torch/extension.h>

#include "kernels/kernels.h"

#define CHECK_DEV(t) TORCH_CHECK((t).is_cuda(), #t " must be a GPU tensor")
#define CHECK_CONTIG(t) TORCH_CHECK((t).is_contiguous(), #t " must be contiguous")
#define CHECK_DT(t, dt) TORCH_CHECK((t).scalar_type() == (dt), #t " has wrong dtype ", (t).scalar_type())
#define CHECK_BF16(t) CHECK_DT(t, at::kBFloat16)

// A consumer of split-K slabs takes exactly one of its bf16 input and the slabs; true: the slabs.
inline bool slabs_given(const c10::optional<at::Tensor>& in, const c10::optional<at::Tensor>& slabs, const char* who) {
  TORCH_CHECK(in.has_value() != slabs.has_value(), who, ": exactly one of the bf16 input and the split-K slabs");
  return slabs.has_value();
}

// `t` as the `splits` fp32 split-K slabs [splits, rows, cols] of a GEMM (oamd::Slabs): what a consumer
// sums in place of its bf16 [rows, cols] input, and what a producer writes. The kernels read the slabs
// 16 B (4 floats) per lane, hence the alignment of the base and of every slab.
inline oamd::Slabs slab_input(const at::Tensor& t, int64_t splits, int64_t rows, int64_t cols, const char* who) {
  TORCH_CHECK(t.is_cuda(), who, ": the split-K slabs must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == at::kFloat, who, ": the split-K slabs must be fp32, got ", t.scalar_type());
  TORCH_CHECK(t.is_contiguous(), who, ": the split-K slabs must be contiguous");
  TORCH_CHECK(splits >= 1 && rows >= 0 && cols >= 0 && t.numel() >= splits * rows * cols, who,
              ": the split-K slabs need splits >= 1 and at least splits * rows * cols elements");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0 && (rows * cols) % 4 == 0, who,
              ": the split-K slabs need a 16-B aligned base and rows * cols % 4 == 0");
  return {t.data_ptr<float>(), (int)splits, rows * cols};
}
