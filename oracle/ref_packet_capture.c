/* ref_packet_capture.c -- TEST INFRASTRUCTURE: lets the reference's packet.c (main loop and decode_task, compiled in
 * place with ax25.c and misc.c into oracle/_ref/libref_packet_dropin.so by oracle/Makefile) run without a network and
 * under a driver that can pace it (tests/dropin/packet_driver.c).  Compiled only where the reference tree is present
 * (it uses the reference's own multicast.h for struct rtp_header / rtp_state / sockcache), together with packet.c.
 *
 * packet.c is built with -Dmain=ref_packet_main -Dexecute_filter_output=cap_execute_filter_output.  Its filter and
 * oscillator calls (create_filter_input / create_filter_output / set_filter / execute_filter_input / set_osc / step_osc /
 * cnrmf) stay undefined in the object and bind to libka9q_hip.so: the reference's decode loop above this library.
 *
 * What multicast.c would provide (it needs <bsd/string.h>, which this image lacks) is bound here instead:
 *   setup_mcast      -- hands out one end of an AF_UNIX SOCK_DGRAM socketpair, one pair for the input (output = 0) and
 *                       one for the decoded frames (output = 1); the driver takes the peer ends from ref_packet_peer();
 *   ntoh_rtp / hton_rtp -- a 12-byte header of this harness's own:  0xA5, marker<<7 | type, seq (LE16), timestamp
 *                       (LE32), ssrc (LE32), the layout ref_audio_capture.c writes.  The RTP header's byte layout
 *                       therefore stays UNPINNED; what is pinned is everything packet.c does with the fields and the
 *                       payload.  The driver packs and unpacks through ref_packet_put_header / ref_packet_get_header, so
 *                       the layout lives in this file alone;
 *   rtp_process      -- this harness's own sequence check: a datagram whose sequence number does not advance is reported
 *                       as a duplicate (-1), everything else as in order (0).  The driver sends in order;
 *   update_sockcache -- nothing to cache for a socketpair.
 * Months and dump_frame come from the reference's misc.c / ax25.c, which build here.
 *
 * The one pacing hook: cap_execute_filter_output(f) posts a counting semaphore and then calls the library's
 * execute_filter_output(f).  decode_task is while(1) and reports nothing per block; a post says "this decoder has finished
 * what it had and is about to wait for the next block".  Without it a driver could complete a second block while a
 * decoder is still on the first, and the filter hand-off (one block number per master) would skip it.
 */
#define _GNU_SOURCE 1
#include <pthread.h>
#include <semaphore.h>
#include <stdint.h>
#include <string.h>
#include <sys/socket.h>
#include <time.h>
#include <unistd.h>

#include "multicast.h"

#undef execute_filter_output                      /* the build renames packet.c's calls; this file means the library's */
struct filter_out;
int execute_filter_output(struct filter_out *);   /* libka9q_hip.so */

static int Pair[2][2] = { { -1, -1 }, { -1, -1 } };   /* [output][0] = packet.c's end, [output][1] = the driver's */
static sem_t Posts;
static long Npost;
static pthread_once_t Once = PTHREAD_ONCE_INIT;

static void init_posts(void){ sem_init(&Posts, 0, 0); }
static void init_once(void){ pthread_once(&Once, init_posts); }

int setup_mcast(char const *target, struct sockaddr *sock, int output, int ttl, int offset){
  (void)target; (void)sock; (void)ttl; (void)offset;
  init_once();
  int const k = output ? 1 : 0;
  if(Pair[k][0] < 0){
    if(socketpair(AF_UNIX, SOCK_DGRAM, 0, Pair[k]) != 0)
      return -1;
    int const big = 1 << 22;
    setsockopt(Pair[k][0], SOL_SOCKET, SO_SNDBUF, &big, sizeof big);
    setsockopt(Pair[k][1], SOL_SOCKET, SO_SNDBUF, &big, sizeof big);
  }
  return Pair[k][0];
}
/* the driver's end of the input (output = 0) or output (output = 1) pair; -1 until packet.c has asked for it */
int ref_packet_peer(int output){
  return Pair[output ? 1 : 0][1];
}

unsigned char *ref_packet_put_header(unsigned char *data, int type, int marker, unsigned seq, uint32_t timestamp, uint32_t ssrc){
  data[0] = 0xA5;
  data[1] = (unsigned char)(((marker & 1) << 7) | (type & 0x7f));
  data[2] = seq & 0xff;
  data[3] = (seq >> 8) & 0xff;
  for(int i = 0; i < 4; i++){
    data[4 + i] = (timestamp >> (8 * i)) & 0xff;
    data[8 + i] = (ssrc >> (8 * i)) & 0xff;
  }
  return data + 12;
}
const unsigned char *ref_packet_get_header(const unsigned char *data, int *type, unsigned *seq, uint32_t *timestamp, uint32_t *ssrc){
  *type = data[1] & 0x7f;
  *seq = data[2] | (data[3] << 8);
  *timestamp = *ssrc = 0;
  for(int i = 0; i < 4; i++){
    *timestamp |= (uint32_t)data[4 + i] << (8 * i);
    *ssrc |= (uint32_t)data[8 + i] << (8 * i);
  }
  return data + 12;
}
unsigned char *hton_rtp(unsigned char *data, struct rtp_header *rtp){
  return ref_packet_put_header(data, rtp->type, rtp->marker, rtp->seq, rtp->timestamp, rtp->ssrc);
}
unsigned char *ntoh_rtp(struct rtp_header *rtp, unsigned char *data){
  int type;
  unsigned seq;
  uint32_t ts, ssrc;
  memset(rtp, 0, sizeof *rtp);
  ref_packet_get_header(data, &type, &seq, &ts, &ssrc);
  rtp->version = RTP_VERS;
  rtp->type = (uint8_t)type;
  rtp->marker = (data[1] >> 7) & 1;
  rtp->seq = (uint16_t)seq;
  rtp->timestamp = ts;
  rtp->ssrc = ssrc;
  return data + 12;
}
int rtp_process(struct rtp_state *state, struct rtp_header *rtp, int samples){
  if(state->init && (int16_t)(rtp->seq - state->seq) < 0){
    state->dupes++;
    return -1;
  }
  state->init = 1;
  state->ssrc = rtp->ssrc;
  state->seq = (uint16_t)(rtp->seq + 1);
  state->timestamp = rtp->timestamp + (uint32_t)samples;
  state->packets++;
  return 0;
}
void update_sockcache(struct sockcache *sc, struct sockaddr *sa){
  (void)sc; (void)sa;
}

int cap_execute_filter_output(struct filter_out *f){
  init_once();
  __atomic_add_fetch(&Npost, 1, __ATOMIC_SEQ_CST);
  sem_post(&Posts);
  return execute_filter_output(f);
}
/* one post, or -1 after timeout_s seconds without one */
int ref_packet_wait_post(int timeout_s){
  init_once();
  struct timespec ts;
  clock_gettime(CLOCK_REALTIME, &ts);
  ts.tv_sec += timeout_s;
  return sem_timedwait(&Posts, &ts);
}
long ref_packet_posts(void){
  return __atomic_load_n(&Npost, __ATOMIC_SEQ_CST);
}
