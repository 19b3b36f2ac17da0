// wase_tree.h -- the split tree of numpy's pairwise sum, walked without recursion: which leaves a piece of n <= 8192
// elements falls into, and in which order their sums are added.  Shared between k_wase_piece_sums (teeflow_wase.hip.h,
// thread 0 of a block runs both walks) and tests/csrc/verify_wase_tree.cpp, which checks every n from 1 to 8192
// against the recursive definition on the CPU.  Plain C++: compiles without HIP.
#ifndef TEEFLOW_WASE_TREE_H
#define TEEFLOW_WASE_TREE_H

#ifndef TF_HD
#define TF_HD
#endif

#define NP_PW_BLOCK 128        // numpy's PW_BLOCKSIZE: a node of at most this many elements is a leaf
#define WASE_MAX_LEAVES 128    // a piece of <= 8192 elements has at most 8192/64 leaves (65 are reached)
#define WASE_TREE_STACK 16     // slots of either walk's stack (8 are reached)

// Called with the index about to be written and the size of the array it goes into.  Nothing in the kernel; the CPU
// verifier defines it before including this file, to refuse an index outside the array and to record the maxima.
#ifndef WASE_TREE_SLOT
#define WASE_TREE_SLOT(i, size) ((void)0)
#endif

// numpy splits n > 128 elements at n/2 rounded down to a multiple of 8
TF_HD inline int np_pw_split(int n) { int n2 = n / 2; return n2 - n2 % 8; }

// Lists the leaves of the tree over [0, n) from left to right: leaf l covers [loff[l], loff[l] + ln[l]).  Returns how
// many there are.
TF_HD inline int wase_tree_leaves(int n, int* loff, int* ln)
{
    int so[WASE_TREE_STACK], sn[WASE_TREE_STACK], sp = 0, nl = 0;
    so[0] = 0; sn[0] = n; sp = 1;
    while (sp > 0) {
        --sp;
        const int o = so[sp], m = sn[sp];
        if (m <= NP_PW_BLOCK) { WASE_TREE_SLOT(nl, WASE_MAX_LEAVES); loff[nl] = o; ln[nl] = m; ++nl; continue; }
        const int n2 = np_pw_split(m);
        WASE_TREE_SLOT(sp + 1, WASE_TREE_STACK);
        so[sp] = o + n2; sn[sp] = m - n2; ++sp;                   // right child below the left one: left is listed first
        so[sp] = o; sn[sp] = n2; ++sp;
    }
    return nl;
}

// Adds the leaf sums lsum[0 .. leaves) up the same tree, left + right at every node: a post-order walk that consumes
// the leaves from left to right.
TF_HD inline float wase_tree_combine(int n, const float* lsum)
{
    int sn[WASE_TREE_STACK], st[WASE_TREE_STACK], sp = 0, k = 0;
    float sl[WASE_TREE_STACK];
    float val = 0.f;
    bool have = false;
    sn[0] = n; st[0] = 0; sp = 1;
    while (sp > 0) {
        const int t = sp - 1;
        if (have) {                                               // a child of the node on top has just been evaluated
            have = false;
            if (st[t] == 1) { WASE_TREE_SLOT(sp, WASE_TREE_STACK); sl[t] = val; st[t] = 2; sn[sp] = sn[t] - np_pw_split(sn[t]); st[sp] = 0; ++sp; }
            else { val = sl[t] + val; have = true; --sp; }
            continue;
        }
        if (sn[t] <= NP_PW_BLOCK) { val = lsum[k++]; have = true; --sp; continue; }
        WASE_TREE_SLOT(sp, WASE_TREE_STACK);
        st[t] = 1; sn[sp] = np_pw_split(sn[t]); st[sp] = 0; ++sp;
    }
    return val;
}

#endif
