"""The arena layouts of the host layer on the CPU: every function of csrc/sbam_layout.h run by a small C++ program on a
null cursor and then over an allocation of exactly the size that pass reported, under the address and
undefined-behaviour sanitizers."""
import os
import subprocess

from conftest import ROOT

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "sbam_layout.h"
using namespace sbam_layout;

// the launcher structs of sbam_internal.h that a layout fills, member for member
struct RecordColumns {
  int64_t *block_pos;
  int32_t *block_off, *block_size, *ref_id, *pos;
  uint32_t *bin_mq_nl, *flag_nc;
  int32_t *l_seq, *next_ref_id, *next_pos, *tlen;
};
struct Counts { u64 *counts, *positions, *rbe, *pair, *scalars, *totals; int32_t *tile_pass0 = nullptr; };
struct IndexStats { u64 *w, *n_mapped, *n_unmapped, *off_beg, *off_end, *n_intv; };
struct TagWalk {
  int32_t nq, nb;
  uint8_t *type, *sub;
  int32_t *rel;
  int64_t *value, *off, ostride, *src;
  u64 *first_bad, *present;
};

struct Col { const uint8_t *p; size_t bytes; };
static std::vector<Col> g_cols;
static int g_bad = 0, g_cases = 0;
static const uint8_t *g_lo, *g_hi;  // the allocation of the pass that writes (null: the null pass)
#define CHECK(cond, ...) do { if (!(cond)) { g_bad++; std::printf("FAIL %s: ", name); std::printf(__VA_ARGS__); \
  std::printf("\n"); } } while (0)

// column p of n elements, as the host layer uses it, aligned as the layout declares: inside the allocation, every
// element written, and remembered for the disjointness check
template <class T>
static void fill(const char *name, T *p, size_t n, size_t align = 256) {
  if (!g_lo) {
    CHECK(p == nullptr, "a column of the null pass is not null");
    return;
  }
  CHECK(p != nullptr, "a null column");
  if (!p) return;
  const uint8_t *b = reinterpret_cast<const uint8_t *>(p);
  CHECK(b >= g_lo && b + n * sizeof(T) <= g_hi, "a column outside the arena");
  CHECK((size_t)(b - g_lo) % align == 0 && align % alignof(T) == 0, "a column not aligned to %zu", align);
  for (size_t i = 0; i < n; i++) p[i] = (T)i;
  g_cols.push_back(Col{b, n * sizeof(T)});
}

// layout(k, name): runs one layout function on k and fills the columns it returned
template <class F>
static void run(const char *name, F layout) {
  g_cases++;
  g_lo = g_hi = nullptr;
  Carve size(nullptr);
  layout(size, name);
  const size_t bytes = size.bytes();
  CHECK(bytes % 256 == 0, "size %zu", bytes);
  // exactly bytes(), 256-B aligned as a device allocation is (an empty arena: one line nobody may write)
  uint8_t *buf = static_cast<uint8_t *>(std::aligned_alloc(256, bytes ? bytes : 256));
  g_lo = buf;
  g_hi = buf + bytes;
  g_cols.clear();
  Carve k(buf);
  layout(k, name);
  CHECK(k.bytes() == bytes, "the passes disagree: %zu and %zu bytes", bytes, k.bytes());
  size_t end = 0;
  for (size_t i = 0; i < g_cols.size(); i++) {
    const Col &a = g_cols[i];
    if (a.bytes) end = end > (size_t)(a.p + a.bytes - buf) ? end : (size_t)(a.p + a.bytes - buf);
    for (size_t j = 0; j < i; j++) {
      const Col &b = g_cols[j];
      CHECK(!a.bytes || !b.bytes || a.p + a.bytes <= b.p || b.p + b.bytes <= a.p, "columns %zu and %zu overlap", j, i);
    }
  }
  CHECK(end <= bytes && bytes - end < 256, "the last column ends at %zu of %zu", end, bytes);
  std::free(buf);
}

int main() {
  const size_t counts[] = {0, 1, 31, 32, 33};  // (at 31..33 an 8-byte column crosses a 256-byte line)
  const size_t geom[] = {1, 2};
  for (size_t n : counts) {
    run("record_cols", [&](Carve &k, const char *name) {
      const RecordColumns r = record_cols<RecordColumns>(k, n);
      fill(name, r.block_pos, n);
      for (int32_t *p : {r.block_off, r.block_size, r.ref_id, r.pos, r.l_seq, r.next_ref_id, r.next_pos, r.tlen})
        fill(name, p, n);
      fill(name, r.bin_mq_nl, n);
      fill(name, r.flag_nc, n);
    });
    for (size_t nblk : geom) {
      run("field_offs", [&](Carve &k, const char *name) {
        const FieldOffs r = field_offs(k, n, nblk);
        for (int64_t *p : r.off) fill(name, p, n + 1);
        fill(name, r.bsum, 4 * nblk);
        fill(name, r.first_bad, 1);
        fill(name, r.totals, 4, 8);
        if (r.first_bad) CHECK(r.totals == r.first_bad + 1, "the totals are not behind the first bad record");
      });
      run("write_sel", [&](Carve &k, const char *name) {
        const WriteSel r = write_sel(k, n, nblk);
        fill(name, r.len, r.stride);
        fill(name, r.cnt, r.stride, 8);
        if (r.len) CHECK(r.cnt == r.len + r.stride && r.stride == n + 2, "the two columns are not one scan's");
        fill(name, r.src, n + 1, 8);
        fill(name, r.bsum, 2 * nblk, 8);
        fill(name, r.tot, 2, 8);
      });
      for (int nq : {1, 32}) {
        for (int nb : {0, 1, 32}) {
          if (nb > nq) continue;
          run("tag_offs", [&](Carve &k, const char *name) {
            TagWalk wa{};
            wa.nq = nq, wa.nb = nb;
            const TagScan r = tag_offs(k, wa, n, nblk, 64);
            CHECK((size_t)wa.ostride >= n + 1 && wa.ostride % 32 == 0, "ostride %lld", (long long)wa.ostride);
            for (int b = 0; b < nb && wa.off; b++) fill(name, wa.off + b * wa.ostride, (size_t)wa.ostride);
            if (!nb) fill(name, wa.off, 0);
            fill(name, wa.src, (size_t)nb * n);
            fill(name, r.bsum, (size_t)nb * nblk);
            fill(name, wa.first_bad, 1);  // one run: what the memset and the copy cover
            fill(name, r.totals, 32, 8);
            fill(name, wa.present, 64 * 32, 8);
            if (wa.first_bad)
              CHECK(reinterpret_cast<u64 *>(r.totals) == wa.first_bad + kTagTotalsAt &&
                        wa.present == wa.first_bad + kTagPresentAt && kTagPresentAt == 33,
                    "the small words are not one run");
          });
        }
      }
    }
    for (int nq : {1, 32}) {
      run("tag_cells", [&](Carve &k, const char *name) {
        TagWalk wa{};
        wa.nq = nq;
        tag_cells(k, wa, n);
        fill(name, wa.type, nq * n);
        fill(name, wa.sub, nq * n);
        fill(name, wa.rel, nq * n);
        fill(name, wa.value, nq * n);
      });
    }
  }
  // byte columns as the fields (5) and the tags (32) take them: 0, 1 and 32 bytes, and columns that are absent
  const int64_t sizes[] = {0, 1, 32, -1};
  for (int ncol : {1, 5, 32}) {
    for (int first = 0; first < 4; first++) {
      for (size_t t : geom) {
        run("byte_col", [&](Carve &k, const char *name) {
          for (int i = 0; i < ncol; i++) {
            const int64_t bytes = sizes[(first + i) % 4];
            if (bytes < 0) continue;
            const ByteCol r = byte_col(k, (size_t)bytes, t);
            fill(name, r.data, (size_t)bytes + 8);  // (+ 8: the gather stores 8 bytes at a time)
            fill(name, r.tiles, 2 * t);
          }
        });
      }
    }
  }
  for (size_t nref : {(size_t)0, (size_t)1}) {
    run("index_words", [&](Carve &k, const char *name) {
      const IndexStats r = index_words<IndexStats>(k, nref);
      fill(name, r.w, 4);  // one run
      for (u64 *p : {r.n_mapped, r.n_unmapped, r.off_beg, r.off_end, r.n_intv}) fill(name, p, nref, 8);
      if (r.w)
        CHECK(r.n_mapped == r.w + 4 && r.n_unmapped == r.n_mapped + nref && r.off_beg == r.n_unmapped + nref &&
                  r.off_end == r.off_beg + nref && r.n_intv == r.off_end + nref, "the words are not one run");
    });
  }
  for (size_t nb : {(size_t)0, (size_t)1, (size_t)33}) {
    run("write_cols", [&](Carve &k, const char *name) {
      const WriteCols r = write_cols(k, nb);
      fill(name, r.pay, nb);
      for (int32_t *p : {r.stored, r.csize, r.usize}) fill(name, p, nb, 4);
    });
  }
  for (size_t batch : {(size_t)1, (size_t)4096}) {
    for (size_t nblk : geom) {
      run("write_sizes", [&](Carve &k, const char *name) {
        const WriteSizes r = write_sizes(k, batch, nblk);
        fill(name, r.tsz, batch + 1);
        fill(name, r.bsum, nblk, 8);
        fill(name, r.tot, 1, 8);
        fill(name, r.n_stored, 1, 8);
      });
    }
  }
  run("count_words", [&](Carve &k, const char *name) {
    const Counts r = count_words<Counts>(k);
    fill(name, r.counts, 21 * 19);  // one run
    fill(name, r.positions, 21, 8);
    fill(name, r.rbe, 21 * 128, 8);
    fill(name, r.pair, 19 * 19, 8);
    fill(name, r.scalars, 4, 8);
    fill(name, r.totals, 19, 8);
    if (r.counts)
      CHECK(r.positions == r.counts + 21 * 19 && r.rbe == r.positions + 21 && r.pair == r.rbe + 21 * 128 &&
                r.scalars == r.pair + 19 * 19 && r.totals == r.scalars + 4, "the words are not one run");
  });
  std::printf("%d cases, %d failures\n", g_cases, g_bad);
  return g_bad ? 1 : 0;
}
"""


def test_layouts_fit_their_arenas(tmp_path):
    """For every layout function and the smallest shapes that can go wrong (record and cell counts 0, 1, 31, 32, 33;
    1 and 32 tag queries with byte columns of 0, 1 and 32 bytes and absent ones; 0 and 1 references, blocks; launch
    geometry counts 1 and 2): the null pass (every column null) and the pass over an allocation of exactly bytes() report the
    same size; every column starts at a multiple of its declared alignment; no two columns overlap; the last column
    ends within bytes(), less than a line before it; the runs that one memset or copy covers are contiguous; and every
    element of every column the layout names is written."""
    src = tmp_path / "layout_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "layout_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "spark-bam_amd", "csrc"), "-o", str(exe),
                    str(src)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert p.stdout.splitlines()[-1].endswith(" cases, 0 failures")
