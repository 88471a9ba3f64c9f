// C-ABI of the MI355X Merkleization engine (include/prysm_merkle.h), built
// with hipcc into libprysm_merkle.so.  This file: version, errors, device
// setup, synthetic inputs and profiling; the subsystems' entry points are in
// hash_api, merkle_api, struct_api, trie_api and multi_api (runtime.hpp).
#include "runtime.hpp"

using namespace mk;
using namespace mk::rt;

extern "C" {

#define MK_STR2(x) #x
#define MK_STR(x) MK_STR2(x)
// MK_BUILD_FLAGS: the -D knobs of a variant build (Makefile `variant`), "default"
// for the shipped library; __graft_entry__.build() refuses any other value
#ifndef MK_BUILD_FLAGS
#define MK_BUILD_FLAGS "default"
#endif
const char* mk_version(void) {
    return "prysm_merkle 0.4 (gfx950; leaf_lock=" MK_STR(MK_LEAF_LOCK) " lock_bars=" MK_STR(MK_LOCK_BARS)
           " elem_lock=1 trie_lock=1 flags=" MK_BUILD_FLAGS ")";
}

const char* mk_strerror(int code) {
    switch (code) {
        case MK_OK: return "ok";
        case MK_EINVAL: return "invalid argument";
        case MK_ENODEV: return "no usable gfx950 device";
        case MK_ENOMEM: return "out of memory";
        case MK_EHIP: return "HIP runtime error";
        case MK_ECOMM: return "RCCL error";
        default: return "unknown error";
    }
}

const char* mk_last_error(void) { return mk::last_error(); }

int mk_device_count(void) { return probe_devices(); }

int mk_init(int device) {
    Scope S(nullptr);
    return S.done(bind_dev(device < 0 ? 0 : device));
}

// ---- synthetic inputs -------------------------------------------------------------
int mk_dev_synth_fill(mk_call* call, void* d_dst, uint64_t nbytes, uint64_t seed, uint64_t word0, void* stream) {
    return dev_entry(call, stream, [&]() -> int {
        if (nbytes % 8) return fail(MK_EINVAL, "nbytes %% 8 != 0");
        if ((uintptr_t)d_dst % 8) return fail(MK_EINVAL, "destination not 8-byte aligned");
        const uint64_t nwords = nbytes / 8;
        if (!nwords) return MK_OK;
        const uint64_t grid = std::min<uint64_t>(ceil_div(nwords, 256), 256 * 64);
        hipLaunchKernelGGL(mk::k_synth, dim3(grid), dim3(256), 0, (hipStream_t)stream, (uint64_t*)d_dst, nwords, seed,
                           word0);
        hipError_t e = hipGetLastError();
        return e == hipSuccess ? MK_OK : fail(MK_EHIP, "k_synth: %s", hipGetErrorString(e));
    });
}

// ---- measurement ----------------------------------------------------------------------
int mk_prof_enable(int on) {
    prof_enable(on != 0);
    return MK_OK;
}

int mk_prof_read(mk_call* call, double* leaf_ms, uint64_t* leaf_launches, double* leaf_perms, double* leaf_hashes) {
    Scope S(call);
    return S.done(prof_read(leaf_ms, leaf_launches, leaf_perms, leaf_hashes));
}

}  // extern "C"
