/* Stand-in for <libssh2.h> (libssh2-dev is not a dependency of this project).  The reference's
 * event-layer header only holds pointers to these three handle types; nothing built here calls
 * into libssh2.  Written from libssh2's man pages: the handles are opaque to callers. */
#ifndef ORC_REF_STANDIN_LIBSSH2_H
#define ORC_REF_STANDIN_LIBSSH2_H
typedef struct orc_standin_ssh2_session LIBSSH2_SESSION;
typedef struct orc_standin_ssh2_channel LIBSSH2_CHANNEL;
typedef struct orc_standin_ssh2_knownhosts LIBSSH2_KNOWNHOSTS;
#endif
