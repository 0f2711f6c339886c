// dmx_isym.inc -- the asm statement of isym_run (dmx_inflate_dev.hip), included twice: with
// ISYM_CELL 0 the LDS ring and the output hold bytes; with ISYM_CELL 1 they hold 16-bit cells
// (a byte value, or a reference into the output before the sw block: the chained decode of
// dictionary streams, dmx_inflate_chained_async).  Only the ring addressing, the ring loads /
// stores and the far-source addressing differ.
#if ISYM_CELL
#define IRADDR(d, s) "v_and_b32 " d ", %[im], " s "\n" "v_lshlrev_b32 " d ", 1, " d "\n"
#define ICSH "1"   // log2 bytes per output position
#define ILITST "ds_write_b16_d16_hi"
#define IRD "ds_read_u16"
#define IWR "ds_write_b16"
// byte offset of lane t's source cell from galn: 2 (op - dist + t) + gmis
#define IFARBASE "s_lshl_b32 s98, s98, 1\n" "s_add_u32 s98, s98, %[gmis]\n" "v_lshl_add_u32 v112, %[lane], 1, s98\n"
#define IFARSTEP "v_add_u32 v112, 0x80, v112\n"
// a match whose source lies wholly before the sw block (dist - op >= len): its cells are the
// references 0x100 + (dist - op - t) - 1, written here; one that runs into the block goes to
// the caller (IX_MATCH)
#define IXREF_BRANCH "s_cbranch_scc1 L_ref%=\n"
#define IREF_BLOCK \
        "L_ref%=:\n" \
        "s_sub_u32 s98, %[dist], %[op]\n" \
        "s_cmp_lt_u32 s98, %[len]\n" \
        "s_cbranch_scc1 L_xmatch%=\n" \
        IFLUSH_PENDING(5) \
        "v_sub_u32 v114, s98, %[lane]\n" \
        "v_add_u32 v114, 0xff, v114\n" \
        "v_add_u32 v113, %[op], %[lane]\n" \
        "s_mov_b32 s99, %[len]\n" \
        "L_rr%=:\n" \
        "v_cmp_gt_u32 vcc, s99, %[lane]\n" \
        "s_and_saveexec_b64 s[92:93], vcc\n" \
        IRADDR("v115", "v113") \
        "ds_write_b16 v115, v114\n" \
        "s_mov_b64 exec, s[92:93]\n" \
        "s_sub_u32 s99, s99, 64\n" \
        "s_cmp_gt_i32 s99, 0\n" \
        "s_cbranch_scc0 L_rrd%=\n" \
        "v_subrev_u32 v114, 64, v114\n" \
        "v_add_u32 v113, 64, v113\n" \
        "s_branch L_rr%=\n" \
        "L_rrd%=:\n" \
        "s_add_u32 %[op], %[op], %[len]\n" \
        "s_cmp_gt_u32 %[bc], 32\n" \
        "s_cbranch_scc1 L_look%=\n" \
        "s_branch L_tok%=\n"
#else
#define IRADDR(d, s) "v_and_b32 " d ", %[im], " s "\n"
#define ICSH "0"
#define ILITST "ds_write_b8_d16_hi"
#define IRD "ds_read_u8"
#define IWR "ds_write_b8"
#define IFARBASE "s_add_u32 s98, s98, %[gmis]\n" "v_add_u32 v112, s98, %[lane]\n"
#define IFARSTEP "v_add_u32 v112, 64, v112\n"
#define IXREF_BRANCH "s_cbranch_scc1 L_xmatch%=\n"
#define IREF_BLOCK
#endif
// one length l of the canonical decode: code = next l bits (MSB-first in s98), d = code -
// first[l]; d < cnt[l] -> s96 = offs[l] + d, s92 = l, L_slf.  F / C / O hold the u16 pairs of
// first / cnt / offs with entry l: its high half for odd l (ISL_HI), the low half for even l.
#define ISL_HI(D, S) "s_lshr_b32 " D ", " S ", 16\n"
#define ISL_LO(D, S) "s_and_b32 " D ", " S ", 0xffff\n"
#define ISL_LEN(T, L, SH, HALF, F, C, O) \
    "s_lshr_b32 s96, s98, " #SH "\n" \
    HALF("s79", F) \
    "s_sub_u32 s96, s96, s79\n" \
    HALF("s79", C) \
    "s_cmp_lt_u32 s96, s79\n" \
    "s_cbranch_scc0 L_" T "n" #L "%=\n" \
    HALF("s79", O) \
    "s_add_u32 s96, s96, s79\n" \
    "s_mov_b32 s92, " #L "\n" \
    "s_branch L_" T "f%=\n" \
    "L_" T "n" #L "%=:\n"
// the canonical decode of a code of 11..15 bits (as ientry_slow) with the ITable at lta + B:
// on success s96 = sym[] index, s92 = code length, branch to L_<T>f; otherwise falls through
#define ISL_DECODE(T, N, B0, B1, B2) \
    IFLUSH_PENDING(N) \
    "v_mov_b32 v124, %[lta]\n" \
    "ds_read_b128 v[112:115], v124 offset:" B0 "\n" /* first[8..15] */ \
    "ds_read_b128 v[116:119], v124 offset:" B1 "\n" /* cnt[8..15] */ \
    "ds_read_b128 v[120:123], v124 offset:" B2 "\n" /* offs[8..15] */ \
    "s_brev_b32 s98, s94\n" /* the next 32 bits, first bit in the MSB */ \
    "s_waitcnt lgkmcnt(0)\n" \
    "v_readfirstlane_b32 s70, v113\n" /* first[10] | first[11] << 16 */ \
    "v_readfirstlane_b32 s71, v114\n" \
    "v_readfirstlane_b32 s72, v115\n" \
    "v_readfirstlane_b32 s73, v117\n" /* cnt */ \
    "v_readfirstlane_b32 s74, v118\n" \
    "v_readfirstlane_b32 s75, v119\n" \
    "v_readfirstlane_b32 s76, v121\n" /* offs */ \
    "v_readfirstlane_b32 s77, v122\n" \
    "v_readfirstlane_b32 s78, v123\n" \
    ISL_LEN(T, 11, 21, ISL_HI, "s70", "s73", "s76") \
    ISL_LEN(T, 12, 20, ISL_LO, "s71", "s74", "s77") \
    ISL_LEN(T, 13, 19, ISL_HI, "s71", "s74", "s77") \
    ISL_LEN(T, 14, 18, ISL_LO, "s72", "s75", "s78") \
    ISL_LEN(T, 15, 17, ISL_HI, "s72", "s75", "s78")
// the symbol: u16 at lta + B + 2 * s96 into s96
#define ISL_SYM(B) \
    "s_lshl_b32 s96, s96, 1\n" \
    "s_add_u32 s96, s96, %[lta]\n" \
    "v_mov_b32 v124, s96\n" \
    "ds_read_u16 v121, v124 offset:" B "\n" \
    "s_waitcnt lgkmcnt(0)\n" \
    "v_readfirstlane_b32 s96, v121\n"
    asm volatile(
        "s_mov_b64 s[94:95], %[bb]\n"
        "s_mov_b32 s89, m0\n"
        "s_mov_b64 s[86:87], exec\n"
        "s_mov_b64 s[84:85], 0\n"
        "global_load_dword v64, %[toff], %[tgl] sc1\n"
        "global_load_dword v65, %[toff], %[tgl] offset:256 sc1\n"
        "global_load_dword v66, %[toff], %[tgl] offset:512 sc1\n"
        "global_load_dword v67, %[toff], %[tgl] offset:768 sc1\n"
        "global_load_dword v68, %[toff], %[tgl] offset:1024 sc1\n"
        "global_load_dword v69, %[toff], %[tgl] offset:1280 sc1\n"
        "global_load_dword v70, %[toff], %[tgl] offset:1536 sc1\n"
        "global_load_dword v71, %[toff], %[tgl] offset:1792 sc1\n"
        "global_load_dword v72, %[toff], %[tgl] offset:2048 sc1\n"
        "global_load_dword v73, %[toff], %[tgl] offset:2304 sc1\n"
        "global_load_dword v74, %[toff], %[tgl] offset:2560 sc1\n"
        "global_load_dword v75, %[toff], %[tgl] offset:2816 sc1\n"
        "global_load_dword v76, %[toff], %[tgl] offset:3072 sc1\n"
        "global_load_dword v77, %[toff], %[tgl] offset:3328 sc1\n"
        "global_load_dword v78, %[toff], %[tgl] offset:3584 sc1\n"
        "global_load_dword v79, %[toff], %[tgl] offset:3840 sc1\n"
        "global_load_dword v80, %[toff], %[tgd] sc1\n"
        "global_load_dword v81, %[toff], %[tgd] offset:256 sc1\n"
        "global_load_dword v82, %[toff], %[tgd] offset:512 sc1\n"
        "global_load_dword v83, %[toff], %[tgd] offset:768 sc1\n"
        "global_load_dword v84, %[toff], %[tgd] offset:1024 sc1\n"
        "global_load_dword v85, %[toff], %[tgd] offset:1280 sc1\n"
        "global_load_dword v86, %[toff], %[tgd] offset:1536 sc1\n"
        "global_load_dword v87, %[toff], %[tgd] offset:1792 sc1\n"
        "global_load_dword v88, %[toff], %[tgd] offset:2048 sc1\n"
        "global_load_dword v89, %[toff], %[tgd] offset:2304 sc1\n"
        "global_load_dword v90, %[toff], %[tgd] offset:2560 sc1\n"
        "global_load_dword v91, %[toff], %[tgd] offset:2816 sc1\n"
        "global_load_dword v92, %[toff], %[tgd] offset:3072 sc1\n"
        "global_load_dword v93, %[toff], %[tgd] offset:3328 sc1\n"
        "global_load_dword v94, %[toff], %[tgd] offset:3584 sc1\n"
        "global_load_dword v95, %[toff], %[tgd] offset:3840 sc1\n"
        "s_mov_b32 s97, 0\n"
        "s_mov_b32 %[len], 0\n"
        "s_mov_b32 %[dist], 0\n"
        "s_waitcnt vmcnt(0)\n"
        // distance bases (m << extra) + 1 beside the distance entries, in v96..v111
        "v_bfe_u32 v116, v80, 28, 2\n"
        "v_bfe_u32 v117, v80, 16, 4\n"
        "v_lshlrev_b32 v116, v117, v116\n"
        "v_add_u32 v96, 1, v116\n"
        "v_bfe_u32 v116, v81, 28, 2\n"
        "v_bfe_u32 v117, v81, 16, 4\n"
        "v_lshlrev_b32 v116, v117, v116\n"
        "v_add_u32 v97, 1, v116\n"
        "v_bfe_u32 v116, v82, 28, 2\n"
        "v_bfe_u32 v117, v82, 16, 4\n"
        "v_lshlrev_b32 v116, v117, v116\n"
        "v_add_u32 v98, 1, v116\n"
        "v_bfe_u32 v116, v83, 28, 2\n"
        "v_bfe_u32 v117, v83, 16, 4\n"
        "v_lshlrev_b32 v116, v117, v116\n"
        "v_add_u32 v99, 1, v116\n"
        "v_bfe_u32 v116, v84, 28, 2\n"
        "v_bfe_u32 v117, v84, 16, 4\n"
        "v_lshlrev_b32 v116, v117, v116\n"
        "v_add_u32 v100, 1, v116\n"
        "v_bfe_u32 v116, v85, 28, 2\n"
        "v_bfe_u32 v117, v85, 16, 4\n"
        "v_lshlrev_b32 v116, v117, v116\n"
        "v_add_u32 v101, 1, v116\n"
        "v_bfe_u32 v116, v86, 28, 2\n"
        "v_bfe_u32 v117, v86, 16, 4\n"
        "v_lshlrev_b32 v116, v117, v116\n"
        "v_add_u32 v102, 1, v116\n"
        "v_bfe_u32 v116, v87, 28, 2\n"
        "v_bfe_u32 v117, v87, 16, 4\n"
        "v_lshlrev_b32 v116, v117, v116\n"
        "v_add_u32 v103, 1, v116\n"
        "v_bfe_u32 v116, v88, 28, 2\n"
        "v_bfe_u32 v117, v88, 16, 4\n"
        "v_lshlrev_b32 v116, v117, v116\n"
        "v_add_u32 v104, 1, v116\n"
        "v_bfe_u32 v116, v89, 28, 2\n"
        "v_bfe_u32 v117, v89, 16, 4\n"
        "v_lshlrev_b32 v116, v117, v116\n"
        "v_add_u32 v105, 1, v116\n"
        "v_bfe_u32 v116, v90, 28, 2\n"
        "v_bfe_u32 v117, v90, 16, 4\n"
        "v_lshlrev_b32 v116, v117, v116\n"
        "v_add_u32 v106, 1, v116\n"
        "v_bfe_u32 v116, v91, 28, 2\n"
        "v_bfe_u32 v117, v91, 16, 4\n"
        "v_lshlrev_b32 v116, v117, v116\n"
        "v_add_u32 v107, 1, v116\n"
        "v_bfe_u32 v116, v92, 28, 2\n"
        "v_bfe_u32 v117, v92, 16, 4\n"
        "v_lshlrev_b32 v116, v117, v116\n"
        "v_add_u32 v108, 1, v116\n"
        "v_bfe_u32 v116, v93, 28, 2\n"
        "v_bfe_u32 v117, v93, 16, 4\n"
        "v_lshlrev_b32 v116, v117, v116\n"
        "v_add_u32 v109, 1, v116\n"
        "v_bfe_u32 v116, v94, 28, 2\n"
        "v_bfe_u32 v117, v94, 16, 4\n"
        "v_lshlrev_b32 v116, v117, v116\n"
        "v_add_u32 v110, 1, v116\n"
        "v_bfe_u32 v116, v95, 28, 2\n"
        "v_bfe_u32 v117, v95, 16, 4\n"
        "v_lshlrev_b32 v116, v117, v116\n"
        "v_add_u32 v111, 1, v116\n"
        // ---- token start: refill (rotating the stream segments when the word is in vnxt)
        "L_tok%=:\n"
        "s_cmp_gt_u32 %[bc], 32\n"
        "s_cbranch_scc1 L_look%=\n"
        "s_sub_u32 s98, %[wi], %[wb]\n"
        "s_cmp_lt_u32 s98, 64\n"
        "s_cbranch_scc1 L_rd%=\n"
        "s_cmp_le_i32 %[wb], %[wrl]\n"
        "s_cbranch_scc0 L_xseg%=\n"
        "s_waitcnt vmcnt(0)\n"
        "v_mov_b32 %[vc], %[vn]\n"
        "s_add_u32 %[wb], %[wb], 64\n"
        "s_sub_u32 s98, s98, 64\n"
        "s_add_u32 s99, %[wb], 64\n"
        "v_add_lshl_u32 v114, %[lane], s99, 2\n"
        "global_load_dword %[vn], v114, %[zb]\n"
        "L_rd%=:\n"
        "s_nop 3\n"
        "v_readlane_b32 s96, %[vc], s98\n"
        "s_lshl_b64 s[92:93], s[96:97], %[bc]\n"
        "s_or_b64 s[94:95], s[94:95], s[92:93]\n"
        "s_add_u32 %[wi], %[wi], 1\n"
        "s_add_u32 %[bc], %[bc], 32\n"
        // ---- literal/length lookup
        "L_look%=:\n"
        "s_bfe_u32 s98, s94, 0x40006\n"
        ILOOK_LL
        "s_bitcmp1_b32 s99, 15\n"
        "s_cbranch_scc1 L_nl%=\n"
        // literal: sym in bits 23:16 (ds_write_b8_d16_hi), every lane the same byte
        "L_lit%=:\n"
        "s_cmp_ge_u32 %[op], %[lim]\n"
        "s_cbranch_scc1 L_lim%=\n"
        "s_and_b32 s98, s99, 31\n"
        "s_lshr_b64 s[94:95], s[94:95], s98\n"
        "s_sub_u32 %[bc], %[bc], s98\n"
        "v_mov_b32 v114, %[op]\n"
        IRADDR("v114", "v114")
        "v_mov_b32 v115, s99\n"
        ILITST " v114, v115\n"
        "s_add_u32 %[op], %[op], 1\n"
        "s_cmp_gt_u32 %[bc], 32\n"
        "s_cbranch_scc1 L_look%=\n"
        "s_branch L_tok%=\n"
        // ---- length (the entry is the s_bfe control of its extra bits)
        "L_nl%=:\n"
        "s_bitcmp1_b32 s99, 14\n"
        "s_cbranch_scc1 L_sl%=\n"
        "L_len%=:\n"
        "s_cmp_ge_u32 %[op], %[lim]\n"
        "s_cbranch_scc1 L_lim%=\n"
        "s_bfe_u32 s91, s94, s99\n"
        "s_lshr_b32 %[len], s99, 23\n"
        "s_add_u32 %[len], %[len], s91\n"
        // the match must fit the capacity (else the caller reports it; nothing consumed yet)
        "s_add_u32 s98, %[op], %[len]\n"
        "s_cmp_gt_u32 s98, %[capr]\n"
        "s_cbranch_scc1 L_xlim%=\n"
        "s_bfe_u32 s98, s99, 0x50008\n"
        "s_lshr_b64 s[94:95], s[94:95], s98\n"
        "s_sub_u32 %[bc], %[bc], s98\n"
        // refill inside the token: the word is in vcur, or it is the first of vnxt and the
        // segments rotate here as at a token start.  Tokens of one size that divides 32 can put
        // every refill of a long stretch here (zlib's zero runs: 2-bit tokens at odd offsets),
        // so this site must rotate too: wi - wb never exceeds 64, and no read goes to a word
        // at or behind wb + 128, which v_readlane would take modulo 64.  Where the run may not
        // rotate (wb > wrl) the length is consumed and the distance is the caller's, refill
        // included (IX_DIST): its ib_word rotates once, with guarded loads.
        "s_cmp_gt_u32 %[bc], 32\n"
        "s_cbranch_scc1 L_dl%=\n"
        "s_sub_u32 s98, %[wi], %[wb]\n"
        "s_cmp_lt_u32 s98, 64\n"
        "s_cbranch_scc1 L_rm%=\n"
        "s_cmp_le_i32 %[wb], %[wrl]\n"
        "s_cbranch_scc0 L_xdist%=\n"
        "s_waitcnt vmcnt(0)\n"
        "v_mov_b32 %[vc], %[vn]\n"
        "s_add_u32 %[wb], %[wb], 64\n"
        "s_sub_u32 s98, s98, 64\n"
        "s_add_u32 s99, %[wb], 64\n"
        "v_add_lshl_u32 v114, %[lane], s99, 2\n"
        "global_load_dword %[vn], v114, %[zb]\n"
        "L_rm%=:\n"
        "s_nop 3\n"
        "v_readlane_b32 s96, %[vc], s98\n"
        "s_lshl_b64 s[92:93], s[96:97], %[bc]\n"
        "s_or_b64 s[94:95], s[94:95], s[92:93]\n"
        "s_add_u32 %[wi], %[wi], 1\n"
        "s_add_u32 %[bc], %[bc], 32\n"
        // ---- distance: entry and base by the same index
        "L_dl%=:\n"
        "s_bfe_u32 s98, s94, 0x40006\n"
        ILOOK_D
        "s_cmp_lt_i32 s99, 0\n"
        "s_cbranch_scc1 L_sd%=\n"
        "L_dc%=:\n"
        "s_bfe_u32 s91, s94, s99\n"
        "s_add_u32 %[dist], s90, s91\n"
        "s_bfe_u32 s98, s99, 0x50008\n"
        "s_lshr_b64 s[94:95], s[94:95], s98\n"
        "s_sub_u32 %[bc], %[bc], s98\n"
        // ---- the copy (op + len <= capr: the length fits), or the caller for a distance before the output
        "s_add_u32 s98, %[op], %[dfl]\n"
        "s_cmp_gt_u32 %[dist], s98\n"
        IXREF_BRANCH
        "s_cmp_gt_u32 %[dist], %[wmax]\n"
        IFAR_BRANCH
        "s_cmp_ge_u32 %[dist], %[len]\n"
        "s_cbranch_scc1 L_cp%=\n"
        "s_cmp_lt_u32 %[dist], 64\n"
        "s_cbranch_scc1 L_per%=\n"
        "L_cp%=:\n"
        IFLUSH_PENDING(1)
        "s_sub_u32 s98, %[op], %[dist]\n"
        "v_add_u32 v112, s98, %[lane]\n"
        "v_add_u32 v113, %[op], %[lane]\n"
        "s_cmp_gt_u32 %[len], 64\n"
        "s_cbranch_scc1 L_cpl%=\n"
        "v_cmp_gt_u32 vcc, %[len], %[lane]\n"      // one round: lanes t < len, left pending
        "s_and_saveexec_b64 s[92:93], vcc\n"
        IRADDR("v114", "v112")
        IRD " v116, v114\n"
        IRADDR("v117", "v113")
        "v_mov_b32 v118, 0\n"
        "s_mov_b64 exec, s[92:93]\n"
        "s_mov_b64 s[84:85], vcc\n"
        "s_add_u32 %[op], %[op], %[len]\n"
        "s_cmp_gt_u32 %[bc], 32\n"
        "s_cbranch_scc1 L_look%=\n"
        "s_branch L_tok%=\n"
        "L_cpl%=:\n"
        "s_mov_b32 s99, %[len]\n"
        "L_cr%=:\n"
        "v_cmp_gt_u32 vcc, s99, %[lane]\n"
        "s_and_saveexec_b64 s[92:93], vcc\n"
        IRADDR("v114", "v112")
        IRD " v114, v114\n"
        IRADDR("v115", "v113")
        ICOPY_WAIT
        IWR " v115, v114\n"
        "s_mov_b64 exec, s[92:93]\n"
        "s_sub_u32 s99, s99, 64\n"
        "s_cmp_gt_i32 s99, 0\n"
        "s_cbranch_scc0 L_cd%=\n"
        "v_add_u32 v112, 64, v112\n"
        "v_add_u32 v113, 64, v113\n"
        "s_branch L_cr%=\n"
        "L_cd%=:\n"
        "s_add_u32 %[op], %[op], %[len]\n"
        "s_branch L_tok%=\n"
        // ---- short period (dist < 64, dist < len): byte t is source byte t mod dist; lane
        // residues start at lane mod dist (float reciprocal, corrected) and advance 64 mod dist
        "L_per%=:\n"
        IFLUSH_PENDING(2)
        "s_sub_u32 s98, %[op], %[dist]\n"
        "v_cvt_f32_u32 v114, %[dist]\n"
        "v_rcp_f32 v114, v114\n"
        "v_cvt_f32_u32 v112, %[lane]\n"
        "v_mul_f32 v112, v112, v114\n"
        "v_cvt_u32_f32 v112, v112\n"
        "v_mul_lo_u32 v112, v112, %[dist]\n"
        "v_sub_u32 v112, %[lane], v112\n"
        "v_cmp_gt_i32 vcc, 0, v112\n"
        "v_add_u32 v114, %[dist], v112\n"
        "v_cndmask_b32 v112, v112, v114, vcc\n"
        "v_subrev_u32 v114, %[dist], v112\n"
        "v_cmp_le_u32 vcc, %[dist], v112\n"
        "v_cndmask_b32 v112, v112, v114, vcc\n"
        "s_mov_b32 s91, 64\n"
        "L_pm%=:\n"
        "s_cmp_lt_u32 s91, %[dist]\n"
        "s_cbranch_scc1 L_pmd%=\n"
        "s_sub_u32 s91, s91, %[dist]\n"
        "s_branch L_pm%=\n"
        "L_pmd%=:\n"
        "v_add_u32 v113, %[op], %[lane]\n"
        "s_mov_b32 s99, %[len]\n"
        "L_pr%=:\n"
        "v_cmp_gt_u32 vcc, s99, %[lane]\n"
        "s_and_saveexec_b64 s[92:93], vcc\n"
        "v_add_u32 v114, s98, v112\n"
        IRADDR("v114", "v114")
        IRD " v114, v114\n"
        IRADDR("v115", "v113")
        "s_waitcnt lgkmcnt(0)\n"
        IWR " v115, v114\n"
        "s_mov_b64 exec, s[92:93]\n"
        "s_sub_u32 s99, s99, 64\n"
        "s_cmp_gt_i32 s99, 0\n"
        "s_cbranch_scc0 L_cd%=\n"
        "v_add_u32 v113, 64, v113\n"
        "v_add_u32 v112, s91, v112\n"
        "v_subrev_u32 v114, %[dist], v112\n"
        "v_cmp_le_u32 vcc, %[dist], v112\n"
        "v_cndmask_b32 v112, v112, v114, vcc\n"
        "s_branch L_pr%=\n"
        // ---- a source older than the ring: from the output already in HBM (flushed, the
        // stores complete), agent-scope dword loads (to L2, past the vector L1)
        "L_far%=:\n"
        IFLUSH_PENDING(3)
        "s_sub_u32 s98, %[op], %[dist]\n"
        IFARBASE
        "v_add_u32 v113, %[op], %[lane]\n"
        "s_cmp_gt_u32 %[len], 64\n"
        "s_cbranch_scc1 L_farl%=\n"
        "v_cmp_gt_u32 vcc, %[len], %[lane]\n"      // one round, left pending
        "s_and_saveexec_b64 s[92:93], vcc\n"
        "v_and_b32 v114, -4, v112\n"
        "global_load_dword v116, v114, %[galn] sc1\n"
        "v_and_b32 v118, 3, v112\n"
        "v_lshlrev_b32 v118, 3, v118\n"
        IRADDR("v117", "v113")
        "s_mov_b64 exec, s[92:93]\n"
        "s_mov_b64 s[84:85], vcc\n"
        "s_add_u32 %[op], %[op], %[len]\n"
        "s_cmp_gt_u32 %[bc], 32\n"
        "s_cbranch_scc1 L_look%=\n"
        "s_branch L_tok%=\n"
        "L_farl%=:\n"
        "s_mov_b32 s99, %[len]\n"
        "L_fr%=:\n"
        "v_cmp_gt_u32 vcc, s99, %[lane]\n"
        "s_and_saveexec_b64 s[92:93], vcc\n"
        "v_and_b32 v114, -4, v112\n"
        "global_load_dword v114, v114, %[galn] sc1\n"
        "v_and_b32 v115, 3, v112\n"
        "v_lshlrev_b32 v115, 3, v115\n"
        "s_waitcnt vmcnt(0)\n"
        "v_lshrrev_b32 v114, v115, v114\n"
        IRADDR("v115", "v113")
        IWR " v115, v114\n"
        "s_mov_b64 exec, s[92:93]\n"
        "s_sub_u32 s99, s99, 64\n"
        "s_cmp_gt_i32 s99, 0\n"
        "s_cbranch_scc0 L_cd%=\n"
        IFARSTEP
        "v_add_u32 v113, 64, v113\n"
        "s_branch L_fr%=\n"
        IREF_BLOCK
        // ---- op reached lim: half the ring is due (fl + FL), flushed here when the caller
        // allows it (fok: a byte/cell ring without the Adler sums, a 16-byte aligned output),
        // then the same symbol again; otherwise (or at the capacity) the caller
        "L_lim%=:\n"
        "s_cmp_eq_u32 s97, %[fok]\n"   // (s97 = 0)
        "s_cbranch_scc1 L_xlim%=\n"
        "s_sub_u32 s98, %[op], %[fl]\n"
        "s_cmp_lt_u32 s98, %[flc]\n"
        "s_cbranch_scc1 L_xlim%=\n"
        "s_and_b32 s98, %[fl], %[flm]\n"   // (a stored block can leave fl off the half-ring grid)
        "s_cmp_lg_u32 s98, 0\n"
        "s_cbranch_scc1 L_xlim%=\n"
        IFLUSH_PENDING(6)
        // positions [fl, fl + FL) = 4 KiB of the ring at LDS (fl mod W) << ICSH, 16 bytes a
        // lane and round, to the output at gfl + (fl << ICSH)
        "s_and_b32 s98, %[fl], %[im]\n"
        "s_lshl_b32 s98, s98, " ICSH "\n"
        "v_lshlrev_b32 v120, 4, %[lane]\n"
        "v_add_u32 v121, s98, v120\n"
        "s_lshl_b32 s98, %[fl], " ICSH "\n"
        "v_add_u32 v120, s98, v120\n"
        "ds_read_b128 v[112:115], v121\n"
        "ds_read_b128 v[116:119], v121 offset:1024\n"
        "s_waitcnt lgkmcnt(0)\n"
        "global_store_dwordx4 v120, v[112:115], %[gfl]\n"
        "global_store_dwordx4 v120, v[116:119], %[gfl] offset:1024\n"
        "s_nop 1\n"   // (store data VGPRs read before they are written again)
        "ds_read_b128 v[112:115], v121 offset:2048\n"
        "ds_read_b128 v[116:119], v121 offset:3072\n"
        "s_waitcnt lgkmcnt(0)\n"
        "global_store_dwordx4 v120, v[112:115], %[gfl] offset:2048\n"
        "global_store_dwordx4 v120, v[116:119], %[gfl] offset:3072\n"
        "s_waitcnt vmcnt(0)\n"   // the stores are done: far-match reads see them
        "s_add_u32 %[fl], %[fl], %[flc]\n"
        "s_add_u32 %[lim], %[fl], %[flc]\n"
        "s_min_u32 %[lim], %[lim], %[capr]\n"
        "s_branch L_look%=\n"
        // ---- a literal/length code longer than the table's IFB bits (entry IVSLOW = ~0): the
        // canonical decode (first code, count and offset per length, from the table's arrays
        // in LDS at lta), as ientry_slow; a literal goes on as the table's literals do, a length
        // or the end of block (or an invalid code) to the caller, nothing consumed.  In the run
        // these literals cost an LDS round trip instead of a return, the caller's decode and the
        // tables' reload at the next entry (≈ 80 returns per block of C3 text).
        "L_sl%=:\n"
        "s_cmp_eq_u32 s99, -1\n"
        "s_cbranch_scc0 L_xsym%=\n"
        ISL_DECODE("sl", 7, "16", "48", "80")
        "s_branch L_xsym%=\n"   // no code of any length: invalid (the caller reports it)
        "L_slf%=:\n"
        ISL_SYM("96")
        "s_cmp_lt_u32 s96, 256\n"
        "s_cbranch_scc0 L_sll%=\n"
        "s_lshl_b32 s99, s96, 16\n"   // a literal in the table's form: byte in 23:16, code length in 4:0
        "s_or_b32 s99, s99, s92\n"
        "s_branch L_lit%=\n"
        "L_sll%=:\n"   // a length in the table's form (iv_ll); the end of block / invalid: the caller
        "s_sub_u32 s96, s96, 257\n"
        "s_cmp_ge_u32 s96, 29\n"
        "s_cbranch_scc1 L_xsym%=\n"
        "s_mov_b32 s79, 0\n"
        "s_cmp_lt_u32 s96, 8\n"
        "s_cbranch_scc1 L_sb0%=\n"
        "s_cmp_eq_u32 s96, 28\n"
        "s_cbranch_scc1 L_sb1%=\n"
        "s_sub_u32 s79, s96, 4\n"
        "s_lshr_b32 s79, s79, 2\n"       // extra bits
        "s_and_b32 s96, s96, 3\n"
        "s_add_u32 s96, s96, 4\n"
        "s_lshl_b32 s96, s96, s79\n"
        "s_add_u32 s96, s96, 3\n"        // base
        "s_branch L_sb2%=\n"
        "L_sb0%=:\n"
        "s_add_u32 s96, s96, 3\n"
        "s_branch L_sb2%=\n"
        "L_sb1%=:\n"
        "s_movk_i32 s96, 0x102\n"
        "L_sb2%=:\n"
        "s_lshl_b32 s99, s96, 23\n"
        "s_lshl_b32 s98, s79, 16\n"
        "s_or_b32 s99, s99, s98\n"
        "s_add_u32 s98, s92, s79\n"
        "s_lshl_b32 s98, s98, 8\n"
        "s_or_b32 s99, s99, s98\n"
        "s_or_b32 s99, s99, s92\n"
        "s_or_b32 s99, s99, 0x8000\n"
        "s_branch L_len%=\n"
        // ---- a distance code longer than IFB bits: the same with the distance ITable (at
        // lta + 672), its entry (iv_d) and base built here; invalid codes to the caller
        "L_sd%=:\n"
        "s_cmp_eq_u32 s99, -1\n"
        "s_cbranch_scc0 L_xdist%=\n"
        ISL_DECODE("sd", 8, "688", "720", "752")
        "s_branch L_xdist%=\n"
        "L_sdf%=:\n"
        ISL_SYM("768")
        "s_cmp_ge_u32 s96, 30\n"
        "s_cbranch_scc1 L_xdist%=\n"
        "s_mov_b32 s79, 0\n"             // extra bits
        "s_mov_b32 s90, s96\n"           // m
        "s_cmp_lt_u32 s96, 4\n"
        "s_cbranch_scc1 L_sd0%=\n"
        "s_sub_u32 s79, s96, 2\n"
        "s_lshr_b32 s79, s79, 1\n"
        "s_and_b32 s90, s96, 1\n"
        "s_add_u32 s90, s90, 2\n"
        "L_sd0%=:\n"
        "s_lshl_b32 s99, s90, 28\n"      // entry: m << 28 | extra << 16 | (clen + extra) << 8 | clen
        "s_lshl_b32 s98, s79, 16\n"
        "s_or_b32 s99, s99, s98\n"
        "s_add_u32 s98, s92, s79\n"
        "s_lshl_b32 s98, s98, 8\n"
        "s_or_b32 s99, s99, s98\n"
        "s_or_b32 s99, s99, s92\n"
        "s_lshl_b32 s90, s90, s79\n"     // base = (m << extra) + 1
        "s_add_u32 s90, s90, 1\n"
        "s_branch L_dc%=\n"
        // ---- exits
        "L_xsym%=:\n"
        "s_mov_b32 %[ex], 1\n"
        "s_branch L_end%=\n"
        "L_xseg%=:\n"
        "s_mov_b32 %[ex], 2\n"
        "s_branch L_end%=\n"
        "L_xlim%=:\n"
        "s_mov_b32 %[ex], 3\n"
        "s_branch L_end%=\n"
        "L_xdist%=:\n"
        "s_mov_b32 %[ex], 4\n"
        "s_branch L_end%=\n"
        "L_xmatch%=:\n"
        "s_mov_b32 %[ex], 5\n"
        "L_end%=:\n"
        IFLUSH_PENDING(4)
        "s_waitcnt vmcnt(0) lgkmcnt(0)\n"
        "s_mov_b32 m0, s89\n"
        "s_mov_b64 %[bb], s[94:95]\n"
        : [bb] "+s"(r.bb), [bc] "+s"(r.bc), [wi] "+s"(r.wi), [wb] "+s"(r.wb), [vc] "+v"(r.vcur),
          [vn] "+v"(r.vnxt), [op] "+s"(op), [ex] "=&s"(ex), [len] "=&s"(len), [dist] "=&s"(dist),
          [lim] "+s"(lim), [fl] "+s"(fl)
        : [capr] "s"(capr), [fok] "s"(fok), [gfl] "s"(gfl), [flc] "n"(W / 2), [flm] "n"(W / 2 - 1), [dfl] "s"(dfl), [toff] "v"(toff), [tgl] "s"(tgl), [tgd] "s"(tgd), [lane] "v"(lane),
          [wrl] "s"(wrl), [zb] "s"(zb), [galn] "s"(galn), [gmis] "s"(gmis), [im] "n"(W - 1), [wmax] "n"(W), [lta] "s"(lta)
        : "memory", "vcc", "scc", "s70", "s71", "s72", "s73", "s74", "s75", "s76", "s77", "s78", "s79", "s84", "s85", "s86", "s87", "s89", "s90", "s91", "s92", "s93", "s94", "s95", "s96", "s97", "s98", "s99",
          "v64", "v65", "v66", "v67", "v68", "v69", "v70", "v71", "v72", "v73", "v74", "v75", "v76", "v77", "v78", "v79", "v80", "v81", "v82", "v83", "v84", "v85", "v86", "v87", "v88", "v89", "v90", "v91", "v92", "v93", "v94", "v95", "v96", "v97", "v98", "v99", "v100", "v101", "v102", "v103", "v104", "v105", "v106", "v107", "v108", "v109", "v110", "v111", "v112", "v113", "v114", "v115", "v116", "v117", "v118", "v119", "v120", "v121", "v122", "v123", "v124");

#undef ISL_HI
#undef ISL_LO
#undef ISL_LEN
#undef ISL_DECODE
#undef ISL_SYM
#undef IRADDR
#undef ICSH
#undef ILITST
#undef IRD
#undef IWR
#undef IFARBASE
#undef IFARSTEP
#undef IXREF_BRANCH
#undef IREF_BLOCK
