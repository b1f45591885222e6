// deflate_test.cc -- syzkaller_amd/csrc/sg_deflate.h under the host compiler and
// its sanitizers (tests/test_db_write.py builds it with
// -fsanitize=address,undefined).  Input file: u32 count, then per input u32
// length and the bytes.  Every input is encoded from a heap copy of exactly
// its length, with tables in a heap block of exactly their size: the count
// phase, the write phase through the counting sink, the write phase into a
// buffer of exactly the counted length, and again into one a byte short (a
// prefix, and nothing outside it).  Then each of the three forms is forced:
// the chosen form's length must be the least of the three, by the pinned tie
// order, and no form may pass the stored bound.  Output file, per input: u8
// form, u64 length, the stream; then for each forced form u64 length and the
// stream.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sg_deflate.h"

static std::vector<uint8_t> read_file(const char* path) {
  std::vector<uint8_t> v;
  FILE* f = fopen(path, "rb");
  if (!f) return v;
  uint8_t buf[1 << 16];
  size_t n;
  while ((n = fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + n);
  fclose(f);
  return v;
}

static uint64_t bound(uint64_t len) {  // sg_deflate_bound, restated
  uint64_t blocks = (len + 65534) / 65535;
  if (blocks < 1) blocks = 1;
  return len + 5 * blocks;
}

// One write phase into an exact-size heap buffer; tables in an exact-size block filled with `fill` first.
static uint8_t* write_exact(const uint8_t* in, uint32_t len, uint64_t n, int force, uint8_t fill, sgdef::Plan* plan) {
  uint8_t* tab = (uint8_t*)malloc(sgdef::kTabBytes);
  memset(tab, fill, sgdef::kTabBytes);
  uint8_t* buf = (uint8_t*)malloc(n ? n : 1);
  sgdef::WriteSink ws(n ? buf : buf + 1, n);
  *plan = sgdef::encode(in, len, sgdef::Tab{tab, 1}, ws, force);
  free(tab);
  if (ws.n != n) {
    free(buf);
    return nullptr;
  }
  return buf;
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: deflate_test IN OUT\n");
    return 2;
  }
  const std::vector<uint8_t> file = read_file(argv[1]);
  if (file.size() < 4) return 2;
  uint32_t count;
  memcpy(&count, file.data(), 4);
  size_t at = 4;
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 2;
  for (uint32_t k = 0; k < count; k++) {
    uint32_t len;
    if (at + 4 > file.size()) return 2;
    memcpy(&len, file.data() + at, 4);
    at += 4;
    if (at + len > file.size()) return 2;
    uint8_t* in = (uint8_t*)malloc(len ? len : 1);
    if (len) memcpy(in, file.data() + at, len);
    const uint8_t* in_exact = len ? in : in + 1;  // (a zero-length input: any load is out of bounds)
    at += len;
    uint8_t* tab = (uint8_t*)malloc(sgdef::kTabBytes);
    memset(tab, 0xA5, sgdef::kTabBytes);
    const sgdef::Plan p = sgdef::plan(in_exact, len, sgdef::Tab{tab, 1});
    memset(tab, 0x5A, sgdef::kTabBytes);
    sgdef::CountSink cs;
    const sgdef::Plan pc = sgdef::encode(in_exact, len, sgdef::Tab{tab, 1}, cs);
    free(tab);
    if (pc.form != p.form || cs.n != p.bytes) {
      fprintf(stderr, "input %u: the counting sink saw %llu bytes, the count phase said %llu\n", k,
              (unsigned long long)cs.n, (unsigned long long)p.bytes);
      return 1;
    }
    sgdef::Plan pw;
    uint8_t* buf = write_exact(in_exact, len, p.bytes, sgdef::kAuto, 0x00, &pw);
    if (!buf || pw.form != p.form) {
      fprintf(stderr, "input %u: the write phase disagrees with the count phase\n", k);
      return 1;
    }
    {  // a span one byte short: the sink clamps, the stream is the same
      const uint64_t n1 = p.bytes - 1;  // (a stream has at least two bytes)
      uint8_t* t3 = (uint8_t*)malloc(sgdef::kTabBytes);
      memset(t3, 0xFF, sgdef::kTabBytes);
      uint8_t* shorter = (uint8_t*)malloc(n1);
      sgdef::WriteSink w3(shorter, n1);
      sgdef::encode(in_exact, len, sgdef::Tab{t3, 1}, w3);
      if (w3.n != p.bytes || memcmp(shorter, buf, n1)) {
        fprintf(stderr, "input %u: the clamped write phase differs\n", k);
        return 1;
      }
      free(shorter);
      free(t3);
    }
    const uint8_t f8 = (uint8_t)p.form;
    fwrite(&f8, 1, 1, out);
    fwrite(&p.bytes, 8, 1, out);
    fwrite(buf, 1, p.bytes, out);
    free(buf);
    uint64_t forced[3];
    for (int f = 0; f < 3; f++) {
      uint8_t* t4 = (uint8_t*)malloc(sgdef::kTabBytes);
      memset(t4, 0x33, sgdef::kTabBytes);
      const sgdef::Plan pf = sgdef::plan(in_exact, len, sgdef::Tab{t4, 1}, f);
      free(t4);
      forced[f] = pf.bytes;
      sgdef::Plan pf2;
      uint8_t* fb = write_exact(in_exact, len, pf.bytes, f, 0xCC, &pf2);
      if (!fb || pf.form != f || pf2.form != f) {
        fprintf(stderr, "input %u: forced form %d: the write phase disagrees with the count phase\n", k, f);
        return 1;
      }
      fwrite(&pf.bytes, 8, 1, out);
      fwrite(fb, 1, pf.bytes, out);
      free(fb);
    }
    // the least of the three; of equal lengths the first of stored, fixed, dynamic
    int want = 0;
    for (int f = 1; f < 3; f++)
      if (forced[f] < forced[want]) want = f;
    if (p.form != want || p.bytes != forced[want] || p.stored != forced[0] || p.fixed != forced[1] ||
        p.dynamic != forced[2]) {
      fprintf(stderr, "input %u: form %d of %llu bytes, the forms take %llu %llu %llu\n", k, p.form,
              (unsigned long long)p.bytes, (unsigned long long)forced[0], (unsigned long long)forced[1],
              (unsigned long long)forced[2]);
      return 1;
    }
    if (forced[0] != bound(len) || sgdef::stored_bytes(len) != bound(len) || p.bytes > bound(len)) {
      fprintf(stderr, "input %u: the bound does not hold\n", k);
      return 1;
    }
    free(in);
  }
  fclose(out);
  printf("PASS %u\n", count);
  return 0;
}
