// Records with list fields (MK_FIELD_LIST; the program: struct_spec.hpp).  A part of the one
// kernel translation unit: merkle_kernels.hip includes it last; it uses k_struct_nested's column helpers.  Built
// as an object of its own it would emit other code for the same text ("Kernel files").
#ifndef MK_KERNEL_UNIT
#error "kernels_struct_list.hip is built through merkle_kernels.hip"
#endif

namespace mk {

// One record per thread, one launch, as k_struct_nested: the same field ops
// and struct closes over the thread's LDS column (column dword q of thread t
// at col[q * NT + t]; NT is a multiple of the 64 banks, so whatever dword a
// lane addresses it stays in bank t % 64 and no two lanes of a wave collide).
//
// A list op opens a loop over the record's own count (clamped to the slot's
// capacity).  Its body hashes item j from the item's cell and stores the
// element hash at its place in a 256-B chunk pair of the column; the end op
// hashes a full pair into a level-1 node and pushes it on a binary-counter
// stack of pending 32-B nodes (also in the column), and after the wave's last
// item runs every lane's tail: the short or single chunk, the 128 zero
// bytes beside an odd node at every level, the length mix-in (hash.go:194-239).
// All of that is one loop around one column hash, whose message length and
// next step differ per lane.
//
// Control flow is uniform per wave: the op index and the item index j are the
// same in every lane, the item loop runs while any lane of the wave has items
// left, and a lane that has none sits masked off (`act`).  No barrier: a
// thread only touches its own column and its own record.
// Dynamic LDS: NT * ls.peak bytes.  The chunk pair alone is 256 B of column, so the 40 KB a workgroup may ask for
// hold 128 threads (a list of one chunk beside a short message) or 64; there is no 256-thread form.
template <uint32_t NT>
__global__ __launch_bounds__(NT) void k_struct_list(const uint8_t* __restrict__ rec, uint64_t n, ListSpec ls,
                                                    uint4* __restrict__ roots) {
    extern __shared__ uint32_t colbase[];
    const uint32_t tid = threadIdx.x;
    uint32_t* col = colbase + tid;
    const uint64_t i = (uint64_t)blockIdx.x * NT + tid;
    const bool live = i < n;
    const uint8_t* r0 = rec + (live ? i : 0) * ls.rec_len;  // n >= 1: a spare lane re-hashes record 0
    const uint8_t* r = r0;  // what the field ops' src counts from: the record, inside a list the item's cell
    bool act = true;        // false: this lane's list is shorter than item j
    uint32_t j = 0, count = 0, pos = 0;  // the open list: item index, the lane's count, the item's byte in the pair
    uint32_t k = 0;
#pragma unroll 1
    while (k < ls.nops) {
        const uint32_t kraw = ls.op[k].kind, src = ls.op[k].src, len = ls.op[k].len;
        const uint32_t kind = kraw & 0xFFu, dst = ls.op[k].dst + ((kraw & kOpItemOut) ? pos : 0u);
        if (kind == kOpList) {  // le32(count) at src, then len cells of `stride` bytes
            count = min(*reinterpret_cast<const uint32_t*>(r0 + src), len);
            j = 0;
            pos = 0;
            act = count > 0;
            r = r0 + src + 4;
            k += 2;  // past the item descriptor
            continue;
        }
        if (kind == kOpListEnd) {
            const uint32_t lsrc = ls.op[src].src, fdst = ls.op[src].dst;
            const uint32_t stride = ls.op[src + 1].src, olen = ls.op[src + 1].len, work = ls.op[src + 1].dst;
            const uint32_t ipc = 128u / olen, ipc2 = 2 * ipc;
            uint32_t* pb = col + (work / 4) * NT;   // the chunk pair
            uint32_t* stk = pb + 64 * NT;           // pending node of level l at dwords [8 (l - 1), 8 l)
            // A lane's tail waits for the wave's last item: every lane then runs it in the same pass of the loop
            // below, where finishing each lane at its own last item would run that loop once per distinct count.
            // (A lane whose list is over keeps its last pair in the column untouched: it is masked off.)
            const bool fin = !__any(j + 1 < count);
            const bool full = act && (j + 1) % ipc2 == 0 && j + 1 < count;
            if (full || fin) {
                const uint32_t p = (fin ? (count ? count - 1 : 0u) : j) / ipc2;  // level-1 nodes pushed before this pair
                const uint32_t items = fin ? (count ? (count - 1) % ipc2 + 1 : 0u) : ipc2;
                uint32_t bytes = items * olen, mlen, lvl = 1, nl = p + 1;  // nl: nodes of level lvl when the list ends here
                bool last = false;                                         // the next hash is the length mix-in
                if (fin && count <= ipc) {  // one chunk (128 zero bytes for no item): Hash(chunk || le64(count) || 0^24)
                    if (count == 0) {
#pragma unroll 1
                        for (uint32_t q = 0; q < 32; ++q) pb[q * NT] = 0;
                        bytes = 128;
                    }
                    const uint32_t lw[8] = {count, 0, 0, 0, 0, 0, 0, 0};
                    col_put_digest<NT>(col, work + bytes, lw);
                    mlen = bytes + 32;
                    last = true;
                } else if (items <= ipc) {  // an odd number of chunks: the last one beside 128 zero bytes
                    const uint32_t q0 = (bytes + 3) / 4;
                    if (bytes % 4) pb[(q0 - 1) * NT] &= (1u << (8 * (bytes % 4))) - 1u;
#pragma unroll 1
                    for (uint32_t q = 0; q < 32; ++q) pb[(q0 + q) * NT] = 0;
                    mlen = bytes + 128;
                } else {
                    mlen = bytes;
                }
                bool go = true;
#pragma unroll 1
                while (go) {
                    uint4 e0, e1;
                    col_digest<NT>(col, work, mlen, e0, e1);
                    const uint32_t dw[8] = {e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w};
                    if (last) {  // the field hash, into the struct's message
                        col_put_digest<NT>(col, fdst, dw);
                        go = false;
                    } else if ((p >> (lvl - 1)) & 1u) {  // a node of this level is pending: their parent
#pragma unroll
                        for (int w = 0; w < 8; ++w) {
                            pb[w * NT] = stk[(8 * (lvl - 1) + w) * NT];
                            pb[(8 + w) * NT] = dw[w];
                        }
                        mlen = 64;
                        ++lvl;
                        nl = (nl + 1) / 2;
                    } else if (!fin) {  // the list goes on: the node waits for its sibling
#pragma unroll
                        for (int w = 0; w < 8; ++w) stk[(8 * (lvl - 1) + w) * NT] = dw[w];
                        go = false;
                    } else if (nl == 1) {  // the root: Hash(root || le64(count) || 0^24)
#pragma unroll
                        for (int w = 0; w < 8; ++w) {
                            pb[w * NT] = dw[w];
                            pb[(8 + w) * NT] = w == 0 ? count : 0u;
                        }
                        mlen = 64;
                        last = true;
                    } else {  // the odd last node of a level with more than one: beside 128 zero bytes
#pragma unroll
                        for (int w = 0; w < 8; ++w) pb[w * NT] = dw[w];
#pragma unroll 1
                        for (uint32_t q = 8; q < 40; ++q) pb[q * NT] = 0;
                        mlen = 160;
                        ++lvl;
                        nl = (nl + 1) / 2;
                    }
                }
            }
            ++j;
            if (!fin) {  // some lane of the wave has item j: the body again
                act = j < count;
                pos = (j % ipc2) * olen;
                r = r0 + lsrc + 4 + (size_t)j * stride;
                k = src + 2;
            } else {
                act = true;
                pos = 0;
                r = r0;
                ++k;
            }
            continue;
        }
        if (!act) {  // an item this lane's list does not have
            ++k;
            continue;
        }
        if (kind == 2) {  // MK_FIELD_RAW, len 1, 2, 4 or 8
            if (((src | dst | len) & 3u) == 0) {
                const uint32_t* A32 = reinterpret_cast<const uint32_t*>(r + src);
                col[(dst / 4) * NT] = A32[0];
                if (len == 8) col[(dst / 4 + 1) * NT] = A32[1];
            } else {
                for (uint32_t b = 0; b < len; ++b) col_put<NT>(col, dst + b, r[src + b], 1);
            }
            ++k;
            continue;
        }
        uint4 d0, d1;
        if (kind == 1 && len % 4 == 0 && len + 4 < 136) {  // MK_FIELD_BYTES in one block
            bytes_block_digest(r + src, len, d0, d1);
        } else if (kind == 1) {  // MK_FIELD_BYTES of any other length
            sponge_rec4(r + src, len, d0, d1);
        } else if (kind == 3) {  // MK_FIELD_VARBYTES: le32(L) at src, then L <= len bytes (its own call, as in k_struct_nested)
            const uint32_t L = min(*reinterpret_cast<const uint32_t*>(r + src), len);
            sponge_rec4(r + src + 4, L, d0, d1);
        } else {  // kOpClose
            col_digest<NT>(col, src, len, d0, d1);
            if (k + 1 == ls.nops) {  // the top-level struct: the record's root
                if (live) {
                    roots[2 * i] = d0;
                    roots[2 * i + 1] = d1;
                }
                break;
            }
        }
        const uint32_t dw[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
        col_put_digest<NT>(col, dst, dw);
        ++k;
    }
}
template __global__ void k_struct_list<128>(const uint8_t*, uint64_t, ListSpec, uint4*);
template __global__ void k_struct_list<64>(const uint8_t*, uint64_t, ListSpec, uint4*);

}  // namespace mk
