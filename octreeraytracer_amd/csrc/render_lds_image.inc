// Piece of render_core.h, not to be included alone: the LDS image -- plane tables, pop table, lds_layout, fill_fast_planes.
namespace ort {
// The fast walk's split-plane tables.  Reversed layout (every kernel at depth <= 8; the
// persistent bounce kernel at depth 9-10): with T = max(256, 2^D) floats, per axis a block
// of 3T floats at float 3T a -- the layout's forward table (entry i = plane i) at its start
// and the same table reversed (entry i = plane 2^D - i) T floats further -- so that a ray
// walking an axis downwards indexes its planes upwards like every other ray (no per-ray
// stride), and every table starts at a multiple of 4T bytes: a node's near plane (index < T)
// is then a byte offset whose low bits are 4 x the index, and the pop moves it to a child's
// with one and/or (fast_step).  The forward table's last entry is the reversed one's first
// (the same plane); the last axis block ends with its reversed table (7T + 2^D + 1 floats in
// all).  Forward layout (the other kernels at depth 9-10, whose LDS holds 256 lanes'
// frames): the forward tables back to back, 2^D + 1 floats each, and a +-4 byte stride per
// axis.  The image a workgroup copies into LDS (lds_layout) is the tables, the rank LUT
// (8 x 256 bytes: in the gap after axis 0's reversed table where it fits, at depth 10) and
// then the frame columns.
ORT_FN bool fast_rev_planes(int depth) { return depth <= 8; }  // the default image's layout
ORT_FN int fast_rev_T(int depth) { return depth <= 8 ? 256 : 1 << depth; }
ORT_FN int fast_axis_floats(int depth, bool rev) { return rev ? 3 * fast_rev_T(depth) : (1 << depth) + 1; }
ORT_FN int fast_axis_floats(int depth) { return fast_axis_floats(depth, fast_rev_planes(depth)); }
ORT_FN int fast_plane_floats(int depth, bool rev) {
    return rev ? 7 * fast_rev_T(depth) + (1 << depth) + 1 : 3 * fast_axis_floats(depth, false);
}
ORT_FN int fast_plane_floats(int depth) { return fast_plane_floats(depth, fast_rev_planes(depth)); }
// The pop table of the depth <= 8 image (the camera walk's fast_pop, Masks64::kPopTable): what
// the pop derives from (hb, D) alone, hb = 8L + 7 - rank the popped mask bit, once per scene
// instead of per lane and step.  Two tables of kPopEntries 16-byte entries, entry hb at
// kPopTableOff + 16 hb in the axis-0 block and kPopTable2 bytes further (the same place of the
// axis-1 block): the tail of the gap after each block's reversed table, which ends at byte
// 4 (T + 2^D + 1) <= 2052, so the image keeps its size and every other byte.  The camera walk
// never pops a level-D leaf (kInlineLeaves), so hb < 8 (D - 1) <= 56; the entries from there
// on are zero.  For a level-(L+1) child of width w4 = 4 << (D-1-L) bytes of plane table:
//   table 1: { m8 = ~(2 w4 - 1), bitA << s, bitB << s, bitC << s },  s = log2 w4, the rank's
//            bit per role axis (A: rank bit 1, B: bit 0, C: bit 2) -- near = (near & m8) | bit << s
//   table 2: { w4, w4 / 2, low word of 1 << hb, high word of 1 << hb }
constexpr int kPopEntries = 56;
constexpr int kPopTableOff = 12 * 256 - 16 * kPopEntries;  // 2176
constexpr int kPopTable2 = 12 * 256;
static_assert(kPopTableOff % 16 == 0 && kPopTableOff >= 4 * (2 * 256 + 1), "the pop table overlaps the reversed table");
ORT_FN bool fast_pop_table(int depth, bool rev) { return rev && depth <= 8; }
ORT_FN uint32_t pop_table_word(int depth, int table, int hb, int k) {
    const int L = hb >> 3;
    if (hb >= 8 * (depth - 1)) return 0u;
    const uint32_t rk = (uint32_t)(~hb) & 7u;
    const uint32_t s = (uint32_t)(depth + 1 - L);
    const uint32_t w4 = 1u << s;
    if (table == 0) {
        if (k == 0) return ~(2u * w4 - 1u);
        const uint32_t bit = k == 1 ? (rk >> 1) & 1u : (k == 2 ? rk & 1u : (rk >> 2) & 1u);
        return bit << s;
    }
    if (k == 0) return w4;
    if (k == 1) return w4 >> 1;
    return (uint32_t)(((uint64_t)1 << hb) >> (k == 2 ? 0 : 32));
}
// The order tables of the depth <= 8 camera walk's child test (Masks64::kOrderBits: child_order_keep):
// two tables of 64 one-byte entries, back to back.  The walk shifts the "false" bits of conditions
// 6k+1 .. 6k+6 below into an index, the first at bit 5; entry index of table k is the AND, over the
// index's set bits, of the complement of that condition's kill set -- rank bits in the reversed
// layout (rank 0 at bit 7; child of rank R: A far <=> R & 2, B far <=> R & 1, C far <=> R & 4).
// A condition kills the ranks with all of `far` set and none of `near`:
//    1 tMA >= E   A near        4 X >= tMA   A far         7 tMA >= tMB  A near, B far   10 cN >= tMA   A far, C near
//    2 tMB >= E   B near        5 X >= tMB   B far         8 tMB >= tMA  A far, B near   11 tMB >= nF   B near, C far
//    3 cN >= E    C near        6 X >= nF    C far         9 tMA >= nF   A near, C far   12 cN >= tMB   B far, C near
// Where the tables live, and why not in the LDS image.  The first form of this test kept them in the
// image, at bytes 2112-2175 of the axis-0 and axis-1 blocks (the gap before each pop table), read by
// two ds_read_u8 whose addresses the index registers completed; it measured 5.8 % at C3
// (profiles/child_order/ab.md).  It was dropped: every byte of the image outside the pop tables is
// pinned -- planes, rank LUT, zero gaps -- by tests/test_pop_table.py, and the workgroup's LDS has no
// other free byte at depth 8.  So the tables are 128 bytes of constant device memory (g_order_tables:
// two cache lines that every wave of a frame shares), read by two global_load_ubyte; the image,
// lds_bytes and the workgroup's LDS are untouched.  This form measures 4.3 % (same file).  They are
// declared here, beside the pop table, because they are the walk's other per-scene-constant table.
constexpr uint32_t order_kill_set(int cond) {  // cond 0..11: condition cond + 1
    // nibble cond: the axes (A 2, B 1, C 4) on which the killed ranks are the far / the near half
    const uint32_t far = (uint32_t)(0x142421412000ull >> (4 * cond)) & 7u;
    const uint32_t near = (uint32_t)(0x414212000412ull >> (4 * cond)) & 7u;
    uint32_t kill = 0;
    for (uint32_t R = 0; R < 8; ++R)
        if ((R & far) == far && (R & near) == 0) kill |= 0x80u >> R;
    return kill;
}
constexpr uint32_t order_table_entry(int table, int index) {
    uint32_t keep = 0xffu;
    for (int j = 0; j < 6; ++j)
        if ((index >> (5 - j)) & 1) keep &= ~order_kill_set(6 * table + j);
    return keep;
}
struct OrderTables {
    uint8_t b[128];  // table 0, then table 1
};
constexpr OrderTables make_order_tables() {
    OrderTables t{};
    for (int i = 0; i < 128; ++i) t.b[i] = (uint8_t)order_table_entry(i >> 6, i & 63);
    return t;
}
#if defined(__HIPCC__)
static __device__ const OrderTables g_order_tables = make_order_tables();
#endif
static constexpr OrderTables kOrderTablesHost = make_order_tables();
struct LdsLayout {
    int lut;     // byte offset of the rank LUT
    int frames;  // byte offset of the frame columns (= the image's size; a multiple of 16)
    int pop;     // byte offset of the pop table (the second one kPopTable2 further); -1: none
};
ORT_FN LdsLayout lds_layout(int depth, bool rev) {
    const int pb = (4 * fast_plane_floats(depth, rev) + 15) & ~15;
    const int T = fast_rev_T(depth);
    LdsLayout l;
    l.pop = fast_pop_table(depth, rev) ? kPopTableOff : -1;
    if (rev && 4 * (2 * T - (1 << depth) - 1) >= 2048) {  // the gap after axis 0's reversed table
        l.lut = 12 * T - 2048;
        l.frames = pb;
    } else {
        l.lut = pb;
        l.frames = pb + 2048;
    }
    return l;
}
ORT_FN void fill_fast_planes(const float* fwd, float* out, int depth, bool rev, int i0 = 0, int step = 1) {
    const int P1 = (1 << depth) + 1;
    const int S = fast_axis_floats(depth, rev);
    const int T = fast_rev_T(depth);
    const int n = fast_plane_floats(depth, rev);
    const bool pop = fast_pop_table(depth, rev);
    for (int o = i0; o < n; o += step) {  // gather form: one writer per entry
        const int a = o / S, r = o - a * S;
        uint32_t u = 0u;  // the gaps: never read as planes
        if (r < P1) u = f2u(fwd[a * P1 + r]);
        else if (rev && r >= T && r - T < P1) u = f2u(fwd[a * P1 + (P1 - 1 - (r - T))]);
        else if (pop && a < 2 && 4 * r >= kPopTableOff) {  // the pop tables, in the gaps of axes 0 and 1
            const int i = r - kPopTableOff / 4;
            u = pop_table_word(depth, a, i >> 2, i & 3);
        }
        // stored as an integer word: several table words are NaN bit patterns
        __builtin_memcpy(out + o, &u, 4);
    }
}
ORT_FN void fill_fast_planes(const float* fwd, float* out, int depth) {
    fill_fast_planes(fwd, out, depth, fast_rev_planes(depth));
}
}  // namespace ort
