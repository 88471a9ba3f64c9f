// The deposit trie handle (mk_trie), shared by trie_api.cpp and trie_admin_api.cpp.
#pragma once
#include "runtime.hpp"

// ---- deposit trie handle -----------------------------------------------------------------
struct mk_trie {
    std::mutex mu;
    int dev = 0;
    uint32_t depth = 32;
    uint64_t cap = 0, count = 0;
    mk::rt::DevBuf levels, root, in, offs, branch;
};
