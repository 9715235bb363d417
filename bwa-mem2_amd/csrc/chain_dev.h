// chain_dev.h -- working records of the chaining kernel (internal).
#pragma once
#include "bm2_dev.h"

struct WSeed {                       // a seed while chains are being built: singly linked in arrival order
    int64_t rbeg;
    int32_t qbeg, len, next, pad;
};

struct WChain {                      // mem_chain_t while it is in the B-tree; first/last seed fields are cached so that
    int64_t pos;                     // test_and_merge never walks the list.  pos = rbeg of the first seed (the key)
    int64_t last_rbeg;
    int32_t first_qbeg, last_qbeg, last_len;
    int32_t n, rid, is_alt, head, tail, w, kept, first, pad;
};

struct BtNode {                      // kbnode_t with t = 5: up to 9 keys (chain indices) and 10 children (node indices).
    int64_t kpos[9];                 // the key's sort field (chain.pos) is kept next to the index so that a search touches the
    int32_t key[9];                  // node only (one memory round trip per level instead of one per probe)
    int32_t ptr[10];
    int32_t is_internal, n, pad;
};

// ---- the COMPACT form of the same records: what k_chain_heavy keeps in LDS for a read whose inputs are staged there (chain.hip: "compact form").
// Every index is at most the tier's capacity (<= 1184), a query position has 15 bits and a seed length 16 (they already travel so in st_ql): 16-bit
// fields throughout, no padding.  Field NAMES are those of the records above, so the chaining code is written once over either form.
struct CChain {                      // WChain in 40 bytes
    int64_t pos, last_rbeg;
    int32_t rid, w;
    int16_t first_qbeg, last_qbeg; uint16_t last_len; int16_t n;
    int16_t head, tail, first; uint8_t is_alt, kept;
};
struct CNode {                       // BtNode in 40 bytes: no kpos -- the chains sit in the same LDS, a probe reads ch[key].pos there
    int16_t key[9];
    int16_t ptr[10];
    uint8_t is_internal, n;
};
struct CSeeds {                      // WSeed without a record: seed t IS the staged seed t (st_rbeg / st_ql), all that is kept is its successor in the chain
    const int64_t *rbeg; const uint32_t *ql; int16_t *next;
};
static_assert(sizeof(CChain) == 40 && sizeof(CNode) == 40, "the LDS carving of k_chain_heavy counts on these");

// where k_chain_finish's outputs go when the chaining kernel's lane writes them itself (chain.hip: chain_finish_one)
struct FinishOut { const int32_t *len; int32_t *srt_out, *reg_seed, *reg_chain; };
