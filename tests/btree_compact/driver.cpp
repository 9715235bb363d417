// tests/btree_compact/driver.cpp -- TEST INFRASTRUCTURE (tests/test_btree_compact.py): the COMPACT form of chain.hip's kbtree restatement (CTree over CNode /
// CChain: 40-byte nodes without a copy of the keys' sort fields, 16-bit keys and pointers -- what k_chain_heavy keeps in LDS) compiled for the host (the
// emulator's rewrite of the source is #included below) and driven by ONE thread beside the memory form it restates (BTree over BtNode / WChain with reg = false)
// over the same insertion sequences.  After EVERY insertion the in-order key sequence must be the same, and so must the lower neighbour kb_intervalp gives for
// any position; the compact nodes must fit the cap / 4 + 2 the kernel carves for them.
#include CHAIN_EMU_CPP
#include <random>
#include <vector>

// n keys from [0, span); `queries` lower-bound look-ups before every insertion.  Returns 0, or the number of the check that failed (detail: where).
extern "C" int bt_compact_check(unsigned seed, int n, long long span, int queries, long long *detail) {
    std::mt19937_64 rng(seed);
    std::vector<WChain> ch((size_t)n);
    std::vector<CChain> cch((size_t)n);
    std::vector<BtNode> nodes((size_t)n + 8);
    std::vector<CNode> cnodes((size_t)n + 8);                      // (room to spare: the bound the kernel counts on is CHECKED below, not relied on)
    std::vector<int32_t> ord((size_t)n + 8);
    std::vector<int16_t> cord((size_t)n + 8);
    BTree a = BTree(); a.nodes = nodes.data(); a.n_nodes = 0; a.n_keys = 0; a.ch = ch.data(); a.reg = false;
    a.root = bt_new(a, 0);
    CTree b; b.nodes = cnodes.data(); b.n_nodes = 0; b.n_keys = 0; b.ch = cch.data();
    b.root = bt_new(b, 0);
    for (int i = 0; i < n; i++) {
        const int64_t k = (int64_t)(rng() % (unsigned long long)span);
        ch[(size_t)i] = WChain(); ch[(size_t)i].pos = k;
        cch[(size_t)i] = CChain(); cch[(size_t)i].pos = k;
        if (i) for (int q = 0; q < queries; q++) {
            const int64_t x = q == 0 ? k : (int64_t)(rng() % (unsigned long long)(span + 2)) - 1;      // (the key about to go in, then anything)
            const int la = bt_lower(a, x), lb = bt_lower(b, x);
            if (la != lb) { detail[0] = i; detail[1] = x; detail[2] = la; detail[3] = lb; return 1; }
        }
        bt_put(a, i, k);
        bt_put(b, i, k);
        const int m = bt_traverse(a, ord.data());
        if (m != i + 1) { detail[0] = i; detail[1] = m; return 2; }
        if (bt_traverse(b, cord.data()) != m) { detail[0] = i; return 3; }
        for (int t = 0; t < m; t++) if (ord[(size_t)t] != (int32_t)cord[(size_t)t]) { detail[0] = i; detail[1] = t; detail[2] = ord[(size_t)t]; detail[3] = cord[(size_t)t]; return 4; }
        if (a.n_nodes != b.n_nodes || a.root != b.root || a.n_keys != b.n_keys) { detail[0] = i; detail[1] = a.n_nodes; detail[2] = b.n_nodes; return 5; }
        if (b.n_nodes > (i + 1) / 4 + 2) { detail[0] = i; detail[1] = b.n_nodes; return 6; }      // the LDS carving: cap / 4 + 2 nodes for cap seeds
    }
    for (int x = 0; x < a.n_nodes; x++) {                         // node for node the same tree (the two forms number their nodes alike)
        const BtNode &p = nodes[(size_t)x]; const CNode &q = cnodes[(size_t)x];
        if (p.n != q.n || p.is_internal != q.is_internal) { detail[0] = x; return 7; }
        for (int t = 0; t < p.n; t++) if (p.key[t] != q.key[t] || p.kpos[t] != cch[(size_t)q.key[t]].pos) { detail[0] = x; detail[1] = t; return 8; }
        if (p.is_internal) for (int t = 0; t <= p.n; t++) if (p.ptr[t] != q.ptr[t]) { detail[0] = x; detail[1] = t; return 9; }
    }
    detail[0] = a.n_nodes; detail[1] = n;
    return 0;
}
