/* packet_driver.c -- TEST INFRASTRUCTURE: runs the reference's packet decoder (oracle/_ref/libref_packet_dropin.so: packet.c's
 * main loop and decode_task, built by oracle/Makefile) above libka9q_hip.so, feeding it PCM datagrams through the
 * socketpairs of oracle/ref_packet_capture.c and collecting the frames it sends.
 *
 *   gcc -std=gnu11 -O2 tests/dropin/packet_driver.c -ldl -lpthread -o packet_driver
 *   packet_driver libka9q_hip.so libref_packet_dropin.so in.bin out.bin
 *
 * in.bin:  records of  uint32 ssrc, uint32 n, n big-endian int16 samples  -- one datagram each, n <= 1000, in the order
 *          they are to be sent.  The first datagram of every ssrc must be shorter than a block (1000 samples).
 * out.bin: int64 posts, int64 blocks, int64 sessions, then per decoded frame, in arrival order:  uint32 ssrc, uint32 len,
 *          len bytes (the datagram's payload after the header).
 *
 * Pacing (the only hook is the semaphore post in front of every execute_filter_output of a decoder thread):
 *   - after the first datagram of an ssrc the driver waits for one post: that session's decode_task has reached its wait;
 *   - after every datagram that completes a block of 1000 for its session it waits for one post: the block is decoded,
 *     its frames are sent, the thread is waiting again.
 * So posts == blocks + sessions exactly when no block was skipped; the test asserts it.
 * The process image is never replaced; the decoder's threads never end (packet.c has no way to stop them), so the main
 * thread leaves through exit(0).
 */
#define _GNU_SOURCE 1
#include <dlfcn.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/socket.h>
#include <unistd.h>

enum { BLOCK = 1000, MAX_SESSIONS = 64, PCM_MONO_PT = 11, WAIT_S = 60 };

static int (*ref_main)(int, char **);
static int (*peer)(int);
static unsigned char *(*put_header)(unsigned char *, int, int, unsigned, uint32_t, uint32_t);
static const unsigned char *(*get_header)(const unsigned char *, int *, unsigned *, uint32_t *, uint32_t *);
static int (*wait_post)(int);
static long (*posts)(void);

static void *run_main(void *arg){
  (void)arg;
  static char *argv[] = { "packet", "-I", "pcm", NULL };
  ref_main(3, argv);
  return NULL;
}
static void *sym(void *h, const char *name){
  void *p = dlsym(h, name);
  if(!p){ fprintf(stderr, "missing %s: %s\n", name, dlerror()); exit(1); }
  return p;
}
static void fail(const char *what){
  fprintf(stderr, "%s\n", what);
  puts("failed");
  fflush(stdout);
  exit(1);
}

int main(int argc, char **argv){
  if(argc != 5){
    fprintf(stderr, "usage: %s libka9q_hip.so libref_packet_dropin.so in.bin out.bin\n", argv[0]);
    return 2;
  }
  if(!dlopen(argv[1], RTLD_NOW | RTLD_GLOBAL)){ fprintf(stderr, "dlopen %s: %s\n", argv[1], dlerror()); return 1; }
  void *h = dlopen(argv[2], RTLD_NOW | RTLD_GLOBAL);
  if(!h){ fprintf(stderr, "dlopen %s: %s\n", argv[2], dlerror()); return 1; }
  ref_main = sym(h, "ref_packet_main");
  peer = sym(h, "ref_packet_peer");
  put_header = sym(h, "ref_packet_put_header");
  get_header = sym(h, "ref_packet_get_header");
  wait_post = sym(h, "ref_packet_wait_post");
  posts = sym(h, "ref_packet_posts");
  FILE *in = fopen(argv[3], "rb"), *out = fopen(argv[4], "wb");
  if(!in || !out){ perror("open"); return 1; }

  pthread_t t;
  pthread_create(&t, NULL, run_main, NULL);
  for(int i = 0; peer(0) < 0 || peer(1) < 0; i++){     /* packet.c:116-131 asks for both before its loop */
    if(i > 30000)
      fail("the decoder never opened its sockets");
    usleep(1000);
  }
  int const fd_in = peer(0), fd_out = peer(1);

  struct { uint32_t ssrc; long sent; unsigned seq; } ses[MAX_SESSIONS];
  int nses = 0;
  long blocks = 0;
  uint32_t hdr[2];
  while(fread(hdr, sizeof hdr, 1, in) == 1){
    uint32_t const ssrc = hdr[0], n = hdr[1];
    unsigned char pkt[12 + 2 * BLOCK];
    if(n == 0 || n > BLOCK || fread(pkt + 12, 2, n, in) != n)
      fail("bad input record");
    int k = 0;
    while(k < nses && ses[k].ssrc != ssrc)
      k++;
    int const first = k == nses;
    if(first){
      if(nses == MAX_SESSIONS || n >= BLOCK)
        fail("too many sessions, or a first datagram that fills a block");
      ses[nses].ssrc = ssrc;
      ses[nses].sent = 0;
      ses[nses].seq = 0;
      nses++;
    }
    put_header(pkt, PCM_MONO_PT, 0, ses[k].seq++, (uint32_t)ses[k].sent, ssrc);
    if(send(fd_in, pkt, 12 + 2 * n, 0) != (ssize_t)(12 + 2 * n))
      fail("send");
    int const completes = ses[k].sent % BLOCK + (long)n >= BLOCK;
    ses[k].sent += n;
    blocks += completes;
    if((first || completes) && wait_post(WAIT_S) != 0)
      fail("no post from the decoder thread");
  }

  long long const head[3] = { posts(), blocks, nses };
  fwrite(head, sizeof head, 1, out);
  for(;;){
    unsigned char pkt[4096];
    ssize_t const r = recv(fd_out, pkt, sizeof pkt, MSG_DONTWAIT);
    if(r < 12)
      break;
    int type;
    unsigned seq;
    uint32_t ts, ssrc;
    const unsigned char *body = get_header(pkt, &type, &seq, &ts, &ssrc);
    uint32_t const rec[2] = { ssrc, (uint32_t)(r - (body - pkt)) };
    fwrite(rec, sizeof rec, 1, out);
    fwrite(body, 1, rec[1], out);
  }
  fclose(out);
  puts("ok");
  fflush(stdout);
  exit(0);
}
