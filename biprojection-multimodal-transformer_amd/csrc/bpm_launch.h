// The launch step of the ONE shape of an entry point -- check, fill, choose, launch -- as the row files (rows_common.h)
// and the attention files (attn_common.h) share it: launch<K>, with_ct, and the dry mode of the lab build.
// Everything sits in the unnamed namespace, as the kernels of those files do: their symbols carry it.
#pragma once
#include <typeinfo>

#include "bpm_common.h"
#include "../../include/bpmult_hip.h"

#ifdef BPM_LAB
// Dry mode of the lab build (prof.hip: bpm_debug_rows_dry / bpm_debug_rows_last): launch() notes what it would have
// launched and launches nothing, so the launch decisions are testable without a GPU (tests/test_rowops_dispatch_cpu.py,
// tests/test_attn_dispatch_cpu.py).
#define BPM_HIDDEN __attribute__((visibility("hidden")))      // shared by the library's files, not exported
extern BPM_HIDDEN int g_bpm_rows_dry;
BPM_HIDDEN void bpm_rows_note(const char* kernel, unsigned grid, unsigned block, const void* aux);
#endif

namespace {
#ifdef BPM_LAB
template <auto K> struct KernelTag {};          // typeid(KernelTag<K>).name() spells the instantiation, arguments included
template <typename T> const void* as_ptr(const T&) { return nullptr; }
template <typename T> const void* as_ptr(T* p) { return (const void*)p; }
#endif

// Every launch of the row and attention files: kernel K on `grid` blocks of `block` threads, no dynamic LDS.
template <auto K, typename... A>
inline int launch(unsigned grid, unsigned block, void* stream, const A&... args) {
#ifdef BPM_LAB
    if (g_bpm_rows_dry) {
        const void* aux = nullptr;                 // the last pointer argument (a workspace, a counter array), if any
        ((aux = as_ptr(args)), ...);
        bpm_rows_note(typeid(KernelTag<K>).name(), grid, block, aux);
        return 0;
    }
#endif
    hipLaunchKernelGGL(K, dim3(grid), dim3(block), 0, (hipStream_t)stream, args...);
    BPM_CHECK_LAUNCH();
    return 0;
}

// f(CT()) with the compute type of `dtype`: bf16_t for BPM_BF16, float for anything else
template <typename F> inline int with_ct(int dtype, F&& f) { return dtype == BPM_BF16 ? f(bf16_t()) : f(float()); }
}  // namespace
