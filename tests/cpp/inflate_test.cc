// inflate_test.cc -- syzkaller_amd/csrc/sg_inflate.h under the host compiler and
// its sanitizers (tests/test_db.py builds it with -fsanitize=address,undefined).
// Input file: u32 count, then per stream u32 length and the bytes.  Every
// stream is decoded from a heap copy of exactly its length, with tables in a
// heap block of exactly their size: once with the count sink, then with the
// write sink into a buffer of exactly the counted length.  Output file, per
// stream: u8 status, u64 consumed, u64 output length, the output bytes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sg_inflate.h"

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

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: inflate_test IN OUT\n");
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
    uint8_t* in_exact = len ? in : in + 1;  // (a zero-length stream: any load is out of bounds)
    at += len;
    uint8_t* tab = (uint8_t*)malloc(sginf::kTabBytes);
    memset(tab, 0xA5, sginf::kTabBytes);
    sginf::CountSink cs;
    uint64_t consumed = 0;
    const int st = sginf::inflate(in_exact, len, sginf::Tab{tab, 1}, cs, consumed);
    const uint64_t olen = st == SG_INFLATE_OK ? cs.n : 0;
    uint8_t* buf = (uint8_t*)malloc(olen ? olen : 1);
    if (st == SG_INFLATE_OK) {
      memset(tab, 0x5A, sginf::kTabBytes);
      sginf::WriteSink ws(olen ? buf : buf + 1, olen);
      uint64_t consumed2 = 0;
      const int st2 = sginf::inflate(in_exact, len, sginf::Tab{tab, 1}, ws, consumed2);
      if (st2 != st || ws.n != cs.n || consumed2 != consumed) {
        fprintf(stderr, "stream %u: the write pass disagrees with the count pass\n", k);
        return 1;
      }
      // a span one byte short: the sink clamps, the decode is the same
      if (olen) {
        uint8_t* shorter = (uint8_t*)malloc(olen - 1 ? olen - 1 : 1);
        sginf::WriteSink w3(shorter, olen - 1);
        uint64_t c3 = 0;
        if (sginf::inflate(in_exact, len, sginf::Tab{tab, 1}, w3, c3) != st || w3.n != cs.n ||
            memcmp(shorter, buf, olen - 1)) {
          fprintf(stderr, "stream %u: the clamped write pass differs\n", k);
          return 1;
        }
        free(shorter);
      }
    }
    const uint8_t s8 = (uint8_t)st;
    const uint64_t c = st == SG_INFLATE_OK ? consumed : 0;
    fwrite(&s8, 1, 1, out);
    fwrite(&c, 8, 1, out);
    fwrite(&olen, 8, 1, out);
    if (olen) fwrite(buf, 1, olen, out);
    free(buf);
    free(tab);
    free(in);
  }
  fclose(out);
  printf("PASS %u\n", count);
  return 0;
}
