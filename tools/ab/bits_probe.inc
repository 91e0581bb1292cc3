// Measurement probes spliced into ya::bits::pass between its two phases (include/solvers.cuh, under -DYA_BITS_MEASUREMENT_PROBES;
// tools/micro/force_ab.hip builds them, -Itools/ab).  NOT product code: both make the kernel's results WRONG on purpose.
//   -DYA_BITS_BALANCE_PROBE   phase 2 as if the wavefront's hits were dealt to its lanes evenly at no cost
//   -DYA_BITS_PHASE1_ONLY     staging + phase 1 alone
// Round 6 (profiles/r06_force_ab.jsonl): 1 M cells, same box, interleaved -- shipped kernel 241 us, phase 1 alone 105 us,
// free balancing 191 us: the upper bound of ANY in-wave balancing scheme is -21 % of the launch (phase 2 138 -> 86 us).
#ifdef YA_BITS_BALANCE_PROBE
    // MEASUREMENT ONLY (tools/micro/force_ab.hip -DYA_BITS_BALANCE_PROBE; results are WRONG by construction): what
    // would phase 2 cost if the wavefront's hits were dealt to its lanes evenly AT NO COST?  Every lane runs the
    // wave-average number of trips -- a lane with fewer hits repeats its last one (arithmetic and loads included),
    // a lane with more drops the rest.  An upper bound on what any in-wave balancing scheme can buy (VERDICT r05
    // item 5); the scheme's own traffic (parking terms in LDS, adding them in order) comes on top.
    {
        int mine = 0;
        for (int w = 0; w < (p + 31) >> 5; w++) mine += __builtin_popcount(words[w * BLOCK]);
        int total = mine;
        for (int o = 32; o >= 1; o >>= 1) total += __shfl_xor(total, o, 64);
        const int trips = (total + 64 * POPS - 1) / (64 * POPS);
        int last_q = 0;
        bool seen = false;  // (a lane without a hit so far has nothing valid to repeat: it sits the trip out)
        for (int trip = 0; trip < trips; trip++) {
            if (cur == 0 && rp < rp_end) {
                cur = nxt;
                wbase += 32;
                rp += BLOCK;
                nxt = *rp;
            }
            // (the shipped loop's shape: the trip's loads first, then its arithmetic)
            Entry<Pt> other[POPS];
            float4 v[POPS];
#pragma unroll
            for (int u = 0; u < POPS; u++) {
                const bool have = cur != 0;
                const int pos = have ? __builtin_clz(cur) : 0;
                cur = have ? cur & (0x7fffffffu >> pos) : cur;
                last_q = have ? wbase + pos : last_q;
                seen = seen || have;
                if (seen) YA_BITS_LOAD(last_q, other[u], v[u])
            }
            if (seen) {
#pragma unroll
                for (int u = 0; u < POPS; u++) YA_BITS_PAIR(other[u], v[u])
            }
        }
        cur = 0;
        rp = rp_end;
    }
#endif
#ifdef YA_BITS_PHASE1_ONLY  // MEASUREMENT ONLY: staging + phase 1 alone (no pair is evaluated; results are wrong)
    F.x += __int_as_float(cur & 1u);  // (keep phase 1 alive)
    cur = 0, rp = rp_end;
#endif
